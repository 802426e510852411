"""ORACLE — test infrastructure, NOT product code.

CPU (torch fp32) restatement of RelightableAvatar's per-ray render hot path, written from the
reference's behaviour, each function citing the reference file:line it follows (paths relative to
/root/reference).  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this module, and only as the checker.  The product path (relightableavatar_amd/) never imports it.

Parity pin: the reference has no tests or golden vectors for this path, so this
oracle is pinned against outputs of the reference itself, generated in the build container by
tests/golden/make_golden.py (imports /root/reference with third-party stubs) and committed as
tests/golden/*.npz.  tests/test_oracle_golden.py checks every stage against those fixtures.
The one third-party op on the path, pytorch3d.ops.knn_points (un-vendored, version unpinned), is
restated as exact brute-force squared-L2 3-NN, ascending (its documented contract); tie order is
unpinned.  Row N3's vertex normals (pytorch3d Meshes.verts_normals, also un-vendored) are restated from the
published algorithm: PARITY UNPINNED for that function; smplx.lbs' bone transforms are pinned through the
reference's own numpy twin (lib/utils/data_utils.py:1004-1069).

Compaction (batch_aware_indexing + multi_gather/multi_scatter, net_utils.py:381-461) is restated
with boolean masks: at B=1 topk(S) of the metric selects exactly the mask-true elements and results
are scattered back, so outputs are order-free.
All tensors here are un-batched (leading B=1 squeezed) unless stated.
"""
import math
from typing import Callable, Optional

import torch
import torch.nn.functional as F


class odict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# ----------------------------------------------------------------------------- operators

def positional_encoding(x: torch.Tensor, L: int) -> torch.Tensor:
    """lib/networks/embedder.py:26-37: [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)]."""
    fb = 2.0 ** torch.linspace(0.0, L - 1, steps=L, dtype=x.dtype)
    xf = x[..., None, None, :] * fb[:, None, None]              # (..., L, 1, 3)
    enc = torch.cat([torch.sin(xf), torch.cos(xf)], dim=-2)     # (..., L, 2, 3)
    return torch.cat([x, enc.reshape(*x.shape[:-1], L * 6)], dim=-1)


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """nn.utils.weight_norm(dim=0): W = g * v / ||v||_row (net_utils.py:1326-1327, base_network.py:145-149)."""
    return v * (g / v.norm(dim=1, keepdim=True))


def softplus100(x):
    return F.softplus(x, beta=100)


def normalize(x: torch.Tensor, eps: float = 1e-8):
    """net_utils.py:1626-1628."""
    return x / (x.norm(dim=-1, keepdim=True) + eps)


def inverse_3x3(R: torch.Tensor, EPS=1e-8):
    """Closed-form adjugate / (det + 1e-8), blend_utils.py:125-165."""
    r00, r01, r02 = R[..., 0, 0], R[..., 0, 1], R[..., 0, 2]
    r10, r11, r12 = R[..., 1, 0], R[..., 1, 1], R[..., 1, 2]
    r20, r21, r22 = R[..., 2, 0], R[..., 2, 1], R[..., 2, 2]
    M = torch.empty_like(R)
    M[..., 0, 0] = r11 * r22 - r21 * r12
    M[..., 1, 0] = -r10 * r22 + r20 * r12
    M[..., 2, 0] = r10 * r21 - r20 * r11
    M[..., 0, 1] = -r01 * r22 + r21 * r02
    M[..., 1, 1] = r00 * r22 - r20 * r02
    M[..., 2, 1] = -r00 * r21 + r20 * r01
    M[..., 0, 2] = r01 * r12 - r11 * r02
    M[..., 1, 2] = -r00 * r12 + r10 * r02
    M[..., 2, 2] = r00 * r11 - r10 * r01
    D = r00 * M[..., 0, 0] + r01 * M[..., 1, 0] + r02 * M[..., 2, 0]
    return M / (D[..., None, None] + EPS)


def sdf_to_sigma(sdf: torch.Tensor, beta: torch.Tensor):
    """Laplace-CDF density, net_utils.py:874-893."""
    x = -sdf
    ind0 = x <= 0
    ind1 = ~ind0
    val0 = 1 / beta * (0.5 * (x * ind0 / beta).exp()) * ind0
    val1 = 1 / beta * (1 - 0.5 * (-x * ind1 / beta).exp()) * ind1
    return val0 + val1


def sdf_to_occ(sdf, beta, dists=0.005):
    """net_utils.py:852-870: occ = 1 - exp(-relu(sigma) * 0.005); sample spacing is ignored (quirk 3)."""
    return 1.0 - torch.exp(-F.relu(sdf_to_sigma(sdf, beta)) * dists)


def volume_rendering(rgb, alpha, eps=1e-8, bg_brightness=0.0):
    """net_utils.py:970-999. rgb (P,S,C), alpha (P,S) -> weights (P,S), map (P,C), acc (P)."""
    expanded = torch.cat([alpha.new_ones(*alpha.shape[:-1], 1), 1.0 - alpha + eps], dim=-1)
    weights = alpha * torch.cumprod(expanded, dim=-1)[..., :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, dim=-2)
    acc_map = torch.sum(weights, -1)
    rgb_map = rgb_map + (1.0 - acc_map[..., None]) * bg_brightness
    return weights, rgb_map, acc_map


def linear2srgb(linear):
    """relight_utils.py:179-192."""
    linear = linear.clip(0.0, 1.0)
    lin = linear * 12.92
    non = 1.055 * torch.pow(linear + 1e-7, 1 / 2.4) - (1.055 - 1)
    return torch.where(linear <= 0.0031308, lin, non)


def gen_light_xyz(env_h, env_w, env_r):
    """relight_utils.py:423-465 (+ sph2cart :370-395)."""
    lat_half = math.pi / env_h / 2
    lng_half = 2 * math.pi / env_w / 2
    lats = torch.linspace(math.pi / 2 - lat_half, -math.pi / 2 + lat_half, env_h)
    lngs = torch.linspace(math.pi - lng_half, -math.pi + lng_half, env_w)
    lngs, lats = torch.meshgrid(lngs, lats, indexing='xy')
    z = env_r * torch.sin(lats)
    x = env_r * torch.cos(lats) * torch.cos(lngs)
    y = env_r * torch.cos(lats) * torch.sin(lngs)
    xyz = torch.stack((x, y, z), dim=-1)
    sin_colat = torch.sin(math.pi / 2 - lats)
    area = 4 * math.pi * sin_colat / torch.sum(sin_colat)
    return xyz, area


def sample_envmap_image(image: torch.Tensor, ray_d: torch.Tensor):
    """relight_utils.py:106-127: equirect bilinear, align_corners=False, border padding. image (H,W,C)."""
    sh = ray_d.shape
    if image.ndim == 4:
        image = image[0]
    d = ray_d.reshape(-1, 3)
    img = image.permute(2, 0, 1).unsqueeze(0)
    theta = torch.arccos(d[:, 2]) - 1e-6
    phi = torch.atan2(d[:, 1], d[:, 0])
    qy = (theta / math.pi) * 2 - 1
    qx = -phi / math.pi
    grid = torch.stack((qx, qy), dim=-1)[None, None]
    rgb = F.grid_sample(img, grid, align_corners=False, padding_mode='border')
    return rgb[0, :, 0].permute(1, 0).reshape(sh)


def shift_envmap(image: torch.Tensor, shift: float):
    """rotate_envmap's shift_image (relight_utils.py:69-85): horizontal float shift with wrap-around, bilinear
    (grid_sample align_corners=False, border padding).  image (H,W,C) -> (H,W,C)."""
    H, W = image.shape[:2]
    i, j = torch.meshgrid(torch.arange(0, H), torch.arange(0, W), indexing='ij')
    gx = (j.float() + 0.5 + shift) % W
    grid = torch.stack([gx / W * 2 - 1, (i.float() + 0.5) / H * 2 - 1], dim=-1)[None]
    return F.grid_sample(image.permute(2, 0, 1)[None], grid, align_corners=False, mode='bilinear', padding_mode='border')[0].permute(1, 2, 0)


def rotate_envmap(novel_lights, index, repeat, probe_width, with_image=False):
    """rotate_envmap relight_utils.py:57-103: (name, rotated probe (eH,eW,3)) — with_image: (name, probe, rotated image or None)."""
    keys = list(novel_lights.keys())
    pr = lambda e, k='probe': e[k][0] if e[k].ndim == 4 else e[k]
    if repeat <= 0:
        e = novel_lights[keys[index]]
        return (keys[index], pr(e), pr(e, 'image') if 'image' in e else None) if with_image else (keys[index], pr(e))
    n_rotation = probe_width * repeat
    i, j = index // n_rotation, index % n_rotation
    e = novel_lights[keys[i]]
    probe = pr(e)
    eW = probe.shape[1]
    uW = eW * repeat
    name, rot = f'{keys[i]}-{j:04d}', shift_envmap(probe, eW / uW * j)
    if not with_image:
        return name, rot
    image = pr(e, 'image') if 'image' in e else None
    return name, rot, (shift_envmap(image, image.shape[1] / uW * j) if image is not None else None)


def probe_axes(cam_R):
    """gen_light_dir relight_utils.py:9-30: camera axes with only the horizontal rotation kept (world z is up/down), then
    the probe's axis convention (y <- -front, z <- -down).  cam_R: (3,3) world-to-camera.  Returns the 3x3 whose columns
    are the axes the probe directions are expressed in."""
    R = cam_R.clone().mT.clone()
    front = R[:, 2].clone()
    down = torch.zeros(3, dtype=R.dtype)
    down[2] = torch.sign(R[2, 1])
    right = normalize(torch.cross(down, front, dim=0))
    front = normalize(torch.cross(right, down, dim=0))
    return torch.stack([right, -front, -down], dim=1)


def add_light_probe(rgb, probe, H, W, cam_R, env_h, env_w, probe_size_ratio):
    """add_light_probe relight_utils.py:38-54 (+ gen_light_dir :26-35): the probe, seen along the camera axes, is pasted
    into the top-left corner.  rgb (H*W,3) -> (H*W,3)."""
    uW = int(W * probe_size_ratio)
    uH = int(uW * env_h / env_w)
    ray_d = normalize(gen_light_xyz(uH, uW, 10.0)[0]) @ probe_axes(cam_R).mT
    out = rgb.reshape(H, W, 3).clone()
    out[:uH, :uW] = sample_envmap_image(probe, ray_d)
    return out.reshape(H * W, 3)


def safe_divide(a, b, eps=1e-8):
    """relight_utils.py:618-633 — mutates its arguments IN PLACE exactly like the reference."""
    a[(a < eps) & (a >= 0)] = eps
    a[(a > -eps) & (a <= 0)] = -eps
    b[(b < eps) & (b >= 0)] = eps
    b[(b > -eps) & (b <= 0)] = -eps
    div = a / b
    div[div != div] = 0.0
    div[(div == math.inf) | (div == -math.inf)] = 0.0
    return div.clip(-1e10, 1e10)


def microfacet_brdf(pts2l, pts2c, normal, albedo, rough, f0=0.02, lambert_only=False, glossy_only=False):
    """Microfacet.__call__ relight_utils.py:484-577 with cancel_cosine=True (default :475).
    pts2l (N,L,3), pts2c (N,3), normal (N,3), albedo (N,3), rough (N,1) -> (N,L,3).
    The in-place aliasing of safe_divide's arguments (cos_theta_m_sq, cos_theta_v) is reproduced."""
    pts2l = F.normalize(pts2l, p=2, dim=-1, eps=1e-7)
    pts2c = F.normalize(pts2c, p=2, dim=-1, eps=1e-7)
    normal = F.normalize(normal, p=2, dim=-1, eps=1e-7)
    l_dot_n = torch.einsum('ijk,ik->ij', pts2l, normal).clip(1e-4, 1)
    v_dot_n = torch.einsum('ij,ij->i', pts2c, normal).clip(1e-4, 1)
    brdf_lambert = albedo[:, None, :].repeat(1, pts2l.shape[1], 1) / math.pi
    brdf_lambert = brdf_lambert * l_dot_n[:, :, None]
    h = F.normalize(pts2l + pts2c[:, None, :], p=2, dim=-1, eps=1e-7)
    # _get_f :610-615
    f = f0 + (1 - f0) * (1 - torch.einsum('ijk,ijk->ij', pts2l, h)) ** 5
    alpha = rough ** 2
    # _get_d :598-608
    cos_m = torch.einsum('ijk,ik->ij', h, normal)
    chi = torch.where(cos_m > 0, 1.0, 0.0)
    cos_m_sq = torch.square(cos_m)
    tan_m_sq = safe_divide(1 - cos_m_sq, cos_m_sq)          # clamps cos_m_sq in place
    denom = math.pi * torch.square(cos_m_sq) * torch.square(alpha ** 2 + tan_m_sq)
    d = safe_divide(alpha ** 2 * chi, denom)
    # _get_g :580-595
    cos_v = torch.einsum('ij,ij->i', normal, pts2c)
    cos_t = torch.einsum('ijk,ik->ij', h, pts2c)
    div = safe_divide(cos_t, cos_v[:, None])                 # clamps cos_v in place (view)
    chi = torch.where(div > 0, 1.0, 0.0)
    cos_v_sq = torch.clip(torch.square(cos_v), 0.0, 1.0)
    tan_v_sq = safe_divide(1 - cos_v_sq, cos_v_sq)
    tan_v_sq = torch.clip(tan_v_sq, 0.0, 1e10)
    denom = 1 + torch.sqrt(1 + alpha ** 2 * tan_v_sq[:, None])
    g = safe_divide(chi * 2, denom)
    l_dot_n = torch.ones_like(l_dot_n)
    denom = 4 * torch.abs(l_dot_n) * torch.abs(v_dot_n)[:, None]
    micro = safe_divide(f * g * d, denom)
    brdf_glossy = micro[:, :, None].repeat(1, 1, 3)
    if lambert_only:
        return brdf_lambert
    if glossy_only:
        return brdf_glossy
    return brdf_glossy + brdf_lambert


def get_near_far_aabb(bounds, ray_o, ray_d, epsilon=1e-8):
    """net_utils.py:1683-1712 (return_raw=True path). bounds (2,3); ray_d is modified on a copy here
    (the reference mutates a gathered temporary, so the caller-visible rays are untouched)."""
    ray_d = ray_d.clone()
    ray_d[(ray_d < epsilon) & (ray_d > -epsilon ** 2)] = epsilon
    ray_d[(ray_d > -epsilon ** 2) & (ray_d < epsilon)] = -epsilon   # matches nothing after the line above
    tmin = (bounds[:1] - ray_o) / ray_d
    tmax = (bounds[1:] - ray_o) / ray_d
    near = torch.minimum(tmin, tmax).max(dim=-1)[0]
    far = torch.maximum(tmin, tmax).min(dim=-1)[0]
    return near, far


def knn3(p1: torch.Tensor, p2: torch.Tensor, K: int = 3, chunk: int = 65536):
    """pytorch3d.ops.knn_points contract: exact squared-L2 K-NN, ascending. p1 (P,3), p2 (N,3).
    Distances are formed as sum((p-v)^2) (not the |p|^2-2pv+|v|^2 expansion) so near-zero values stay exact."""
    # top-k per block of rows (it is a per-row operation): blocks of 512 rows keep the (rows x N) distance matrix of every elementwise pass
    # in cache (14 MB against 6890 vertices; 4096-row blocks ran 5.7 x slower, and the ground-pass tests spend most of their time here)
    d2s, idxs = [], []
    step = 512 if p1.shape[0] > 512 else max(p1.shape[0], 1)
    for i in range(0, max(p1.shape[0], 1), step):
        q = p1[i:i + step]
        # (dx^2 + dy^2) + dz^2 coordinate by coordinate: the same sums in the same order as ((q - v) ** 2).sum(-1), bit for bit, without the
        # (rows, N, 3) temporaries (the ground-pass tests spend most of their time here)
        d = q[:, 0:1] - p2[None, :, 0]
        d *= d
        for c in (1, 2):
            t = q[:, c:c + 1] - p2[None, :, c]
            t *= t
            d += t
        d2, idx = d.topk(K, dim=-1, largest=False, sorted=True)
        d2s.append(d2)
        idxs.append(idx)
    return torch.cat(d2s), torch.cat(idxs)


def knn_with_filter(pts, verts, norm, K, th):
    """lib/utils/sample_utils.py:164-194 (cfg.use_geodesic_filter = False): ONE distance per point, sqrt(mean_k d_k^2) with the sign
    of max_k sign((x - v_k) . n_k), and the K neighbours as found.  The reference asks knn_points for unsorted neighbours and takes
    column 0 as the closest for the fine mask (:186); the neighbours here are ascending, as in geodesic_knn."""
    d2, nn = knn3(pts, verts, K)
    dot = ((pts[:, None, :] - verts[nn]) * norm[nn]).sum(-1)
    sdf_batch = d2.mean(dim=-1, keepdim=True).sqrt() * dot.sign().max(dim=-1, keepdim=True)[0]
    mask = d2[:, 0] < th ** 2
    return sdf_batch, nn, mask, d2, nn


def geodesic_knn(pts, verts, norm, tverts, K, th, use_geodesic_filter=True):
    """lib/utils/sample_utils.py:103-162.  Returns full-set (sdf_batch, nn_batch), the fine mask
    (d2_min < th^2, :133) and the per-point geodesically filtered (d2, nn) (valid where mask)."""
    if not use_geodesic_filter:
        return knn_with_filter(pts, verts, norm, K, th)
    d2, nn = knn3(pts, verts, K)
    dist = d2.sqrt()
    dot = ((pts[:, None, :] - verts[nn]) * norm[nn]).sum(-1)
    sdf_batch = dist * dot.sign()
    mask = d2[:, 0] < th ** 2
    tv = tverts[nn]
    msk = (tv - tv[:, :1]).pow(2).sum(-1) < th ** 2
    d2f = torch.where(msk, d2, d2[:, :1])
    nnf = torch.where(msk, nn, nn[:, :1])
    sdf_batch = torch.where(msk, sdf_batch, sdf_batch[:, :1])
    nn_batch = nnf
    return sdf_batch, nn_batch, mask, d2f, nnf


# ----------------------------------------------------------------------------- networks

GRAD_SCALE = 16.0       # csrc/ra_k4.hpp: the backward pass carries every gradient times 2^4 (f16 headroom)


class _KernelTransposedProduct(torch.autograd.Function):
    """an emulated nn.Linear whose forward value `y` was computed elsewhere; backward = the K4 kernel's transposed product:
    u = W^T q(delta * GRAD_SCALE) / GRAD_SCALE with the weights `wb` as the backward stream packs them, fp32 accumulate.
    dt None: no rounding of delta (the SDF head's row 0 seeds the backward pass in fp32).  stats: largest |delta * GRAD_SCALE|
    and how many nonzero deltas fall below the operand type's smallest normal value."""

    @staticmethod
    def forward(ctx, x, y, wb, dt, stats):
        ctx.save_for_backward(wb)
        ctx.dt, ctx.stats = dt, stats
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        wb, = ctx.saved_tensors
        if ctx.dt is not None:
            gs = g * GRAD_SCALE
            if ctx.stats is not None:
                a = gs.abs()
                nz = a > 0
                ctx.stats['max_abs'] = max(ctx.stats.get('max_abs', 0.0), float(a.max()) if a.numel() else 0.0)
                ctx.stats['n_nonzero'] = ctx.stats.get('n_nonzero', 0) + int(nz.sum())
                ctx.stats['n_subnormal'] = ctx.stats.get('n_subnormal', 0) + int((nz & (a < torch.finfo(ctx.dt).tiny)).sum())
            g = gs.to(ctx.dt).float() / GRAD_SCALE
        return g @ wb, None, None, None, None


class _TapedSoftplus(torch.autograd.Function):
    """Softplus(beta=100) whose derivative is the K4 kernel's: sigma'(z) = 1 - 2^-y' from the activation the forward kernel
    tapes, y' = y * SP_SCALE rounded to the operand type (EPI_GRAD_SP)"""

    @staticmethod
    def forward(ctx, z, dt):
        y = softplus100(z)
        ctx.save_for_backward((y * OracleNet.SP_SCALE).to(dt).float())
        return y

    @staticmethod
    def backward(ctx, g):
        yq, = ctx.saved_tensors
        return g * (1.0 - torch.exp2(-yq)), None


class _SignMaskRelu(torch.autograd.Function):
    """ReLU whose derivative is the K4 kernel's: the gradient passes where the pre-activation's sign bit is clear (EPI_GRAD_RELU)"""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(~torch.signbit(z))
        return F.relu(z)

    @staticmethod
    def backward(ctx, g):
        m, = ctx.saved_tensors
        return g * m


class OracleNet:
    """Plain-weight view of the reference state_dict + frame-independent ops."""

    def __init__(self, sd: dict, cfg, emulate: Optional[str] = None, kernel_like: bool = False, emulate_backward: bool = False):
        """emulate: None (fp32, the reference's arithmetic) | 'f16' | 'bf16' — every nn.Linear of the MLPs rounds its input
        and its weight to that type and accumulates in fp32 (what a 16-bit-operand MFMA does; SURVEY.md:305 probe).  It is the
        floor any 16-bit-operand kernel can reach.  kernel_like additionally mirrors the HIP kernels' two deliberate
        deviations from a plain operand rounding: the pose condition enters through an fp32 per-frame bias (never rounded), and
        the coordinate / frequency-0 encoding channels of the SDF net's two encoding-fed layers are carried as hi + lo pairs.
        emulate_backward (with emulate 'f16' | 'bf16' and kernel_like): autograd through the geometry networks (d sdf / d bpts,
        the normals) rounds the way the reverse-mode kernel K4 does (csrc/ra_k4.hpp, backward stream of csrc/ra_pack.cpp) and in
        no other way: every transposed product takes q(delta * GRAD_SCALE) and the UNSCALED weights as packed (the SDF net's
        1/sqrt(2) fold included, the hi + lo duplicates of the encoding columns not), fp32 accumulate; sigma' = 1 - 2^-q(y') from
        the taped scaled activation; ReLU masks from the pre-activations' sign bits; the SDF head's row 0 seeds in fp32; the
        residual net's seed resd_limit (1 - tanh^2) g is rounded like a delta; the encoding Jacobian and the final sums are fp32.
        After each residual-net evaluation `relu_margin` holds per point the smallest |pre-activation| / rounding noise over the
        2048 ReLU units (noise: u sqrt(sum (w x)^2) of the rounded operands, u the unit roundoff — the rms of the operand rounding's
        error): where it is below ~1 a ReLU mask may differ between two arithmetics, and the gradient with it by a kink's height.
        `delta_stats` collects the range of the rounded deltas."""
        self.cfg = cfg
        # 'f64acc': every nn.Linear is evaluated in float64 and rounded once to fp32 — a DIFFERENTLY ASSOCIATED (and more accurate)
        # fp32 arithmetic than the reference's BLAS sums: what it changes in a frame is what fp32 itself cannot pin (tools/precision_tiers.py).
        # 'f16x2': operands as f16 hi + lo pairs, three products hi*hi + lo*hi + hi*lo, fp32 accumulate — the compensated tier of
        # the HIP kernels (K3C / K4C).
        # 'f16w2' / 'f16a2': only ONE operand side as a hi + lo pair (two products per k-step): the weights (a constant, systematic
        # perturbation of the field when rounded) resp. the activations (rounding noise that is white from ray to ray) — which half of
        # the plain-f16 error reaches the pixels (tools/precision_tiers.py)
        self.f64acc = emulate == 'f64acc'
        self.split = emulate == 'f16x2'
        self.half_split = {'f16w2': 'w', 'f16a2': 'a'}.get(emulate)
        self.emulate = {None: None, 'f32': None, 'f64acc': None, 'f16': torch.float16, 'bf16': torch.bfloat16, 'f16x2': torch.float16,
                        'f16w2': torch.float16, 'f16a2': torch.float16}[emulate]
        self.kernel_like = bool(kernel_like) and self.emulate is not None
        self.emulate_backward = bool(emulate_backward)
        if self.emulate_backward and not (emulate in ('f16', 'bf16') and self.kernel_like):
            raise ValueError("emulate_backward needs emulate='f16' | 'bf16' and kernel_like=True")
        self.relu_margin = None
        self.delta_stats = {}
        self.shadow_net = None           # tiered precision: another OracleNet (same weights) that answers the light-visibility queries
        f = lambda k: sd[k].detach().float().clone()
        self.resd = [(f(f'residual_deformation_network.mlp.linears.{i}.weight'),
                      f(f'residual_deformation_network.mlp.linears.{i}.bias')) for i in range(9)]
        p = 'signed_distance_network.mlp.lin'
        self.sdf = [(fold_weight_norm(f(f'{p}{l}.weight_g'), f(f'{p}{l}.weight_v')), f(f'{p}{l}.bias')) for l in range(9)]
        self._beta = f('signed_distance_network._beta')
        self.color = [(fold_weight_norm(f(f'render_network.l{i}.weight_g'), f(f'render_network.l{i}.weight_v')),
                       f(f'render_network.l{i}.bias')) for i in range(5)]
        self.relight = 'albedo_network.linears.0.weight' in sd
        if self.relight:
            self.albedo = [(f(f'albedo_network.linears.{i}.weight'), f(f'albedo_network.linears.{i}.bias')) for i in range(3)]
            self.rough = [(f(f'roughness_network.linears.{i}.weight'), f(f'roughness_network.linears.{i}.bias')) for i in range(3)]
            self.global_env_map_ = f('global_env_map_')
            self.light_xyz = f('light_xyz_')
            self.light_area = f('light_area')
            self.light_sharp = f('light_sharp')

    @property
    def beta(self):
        return self._beta.clamp(1e-9, 1e6)    # base_network.py:74-76

    @property
    def global_env_map(self):
        g = self.global_env_map_
        return F.softplus(g.expand(*g.shape[:2], 3))   # relight_network.py:86-89

    def _q(self, t):
        return t if self.emulate is None else t.to(self.emulate).float()

    SP_SCALE = 144.26950408889634        # beta * log2(e): the kernels run the softplus layers in the domain y' = y * SP_SCALE

    def lin(self, x, w, b, exact_cols=None, hilo_cols=None, scaled_x=False, scaled_w_cols=None, seed=False):
        """_lin below; with emulate_backward, autograd through it is the K4 kernel's transposed product (seed: the SDF head,
        whose row 0 enters the backward pass in fp32)"""
        if self.emulate_backward and torch.is_grad_enabled() and x.requires_grad:
            with torch.no_grad():
                y = self._lin(x.detach(), w, b, exact_cols, hilo_cols, scaled_x, scaled_w_cols)
            return _KernelTransposedProduct.apply(x, y, w if seed else self._q(w), None if seed else self.emulate, self.delta_stats)
        return self._lin(x, w, b, exact_cols, hilo_cols, scaled_x, scaled_w_cols)

    def _relu(self, x):
        return _SignMaskRelu.apply(x) if self.emulate_backward else F.relu(x)

    def _softplus(self, x):
        return _TapedSoftplus.apply(x, self.emulate) if self.emulate_backward else softplus100(x)

    def _lin(self, x, w, b, exact_cols=None, hilo_cols=None, scaled_x=False, scaled_w_cols=None):
        """F.linear with the operand rounding of the emulation mode.  exact_cols: slice of input columns that stay fp32
        (the kernel folds them into a bias); hilo_cols: index list of input columns fed as hi + lo pairs against the same
        rounded weight (residual of the first rounding rounded again).  kernel_like only: scaled_x — the input is rounded as
        x * SP_SCALE (hidden activations of the softplus net live in the scaled domain); scaled_w_cols — these weight columns
        are rounded as w * SP_SCALE (they are fed by the unscaled encoding and carry the factor)."""
        if self.f64acc:
            return F.linear(x.double(), w.double(), b.double()).float()
        if self.emulate is None:
            return F.linear(x, w, b)
        S = self.SP_SCALE
        if self.split:
            # hi + lo pairs of both operands in the domain the kernel holds them in (scaled hidden activations / scaled encoding-fed
            # weight columns); the pose-condition columns stay fp32 (folded into a bias)
            xs, ws = x, w
            if self.kernel_like and scaled_x:
                n_h = x.shape[-1] if scaled_w_cols is None else scaled_w_cols.start
                xs = torch.cat([x[..., :n_h] * S, x[..., n_h:]], dim=-1)      # y' = W_h (S x_h) + (S W_pe) x_pe = S y
            if self.kernel_like and scaled_w_cols is not None:
                ws = ws.clone()
                ws[:, scaled_w_cols] = ws[:, scaled_w_cols] * S
            xh, wh = self._q(xs), self._q(ws)
            xl, wl = self._q(xs - xh), self._q(ws - wh)
            if self.kernel_like and exact_cols is not None:
                xh, xl, wh, wl = xh.clone(), xl.clone(), wh.clone(), wl.clone()
                xh[..., exact_cols], wh[:, exact_cols] = xs[..., exact_cols], ws[:, exact_cols]
                xl[..., exact_cols], wl[:, exact_cols] = 0, 0
            y = F.linear(xh, wh) + F.linear(xl, wh) + F.linear(xh, wl)
            if self.kernel_like and (scaled_x or scaled_w_cols is not None):
                y = y / S
            return y + b
        if self.kernel_like and scaled_x:
            n_h = x.shape[-1] if scaled_w_cols is None else scaled_w_cols.start
            xq = torch.cat([self._q(x[..., :n_h] * S) / S, self._q(x[..., n_h:])], dim=-1)
        else:
            xq = self._q(x)
        wq = self._q(w)
        if self.kernel_like and scaled_w_cols is not None:
            wq = wq.clone()
            wq[:, scaled_w_cols] = self._q(w[:, scaled_w_cols] * S) / S
        if self.half_split == 'w':          # weights as hi + lo: rounded twice (22 bits)
            wq = wq + self._q(w - wq)
        elif self.half_split == 'a':        # activations as hi + lo
            xq = xq + self._q(x - xq)
        if self.kernel_like and hilo_cols is not None:
            xq = xq.clone()
            xq[..., hilo_cols] = xq[..., hilo_cols] + self._q(x[..., hilo_cols] - xq[..., hilo_cols])
        if self.kernel_like and exact_cols is not None:
            xq = xq.clone()
            xq[..., exact_cols] = x[..., exact_cols]
            wq = wq.clone()
            wq[:, exact_cols] = w[:, exact_cols]
        return F.linear(xq, wq, b)

    def residuals(self, bpts, cond):
        """base_network.py:34-42 + MLP net_utils.py:1263-1273 (ReLU, skip at 4 as cat([x, input]))."""
        pe = positional_encoding(bpts, self.cfg.xyz_res)
        inp = torch.cat([pe, cond.expand(bpts.shape[0], -1)], dim=-1)
        x = inp
        margin = None
        for i, (w, b) in enumerate(self.resd):
            if i == 4:
                x = torch.cat([x, inp], dim=-1)
            c0 = (0 if i == 0 else 256) + pe.shape[-1]
            xin = x
            x = self.lin(x, w, b, exact_cols=slice(c0, c0 + cond.shape[-1]) if i in (0, 4) else None)
            if i < 8:
                if self.emulate_backward:
                    with torch.no_grad():
                        u = torch.finfo(self.emulate).eps / 2          # unit roundoff
                        noise = u * (self._q(xin.detach()).square() @ self._q(w).square().T).sqrt()
                        m = (x.detach().abs() / noise.clamp_min(1e-30)).amin(dim=-1)
                        margin = m if margin is None else torch.minimum(margin, m)
                x = self._relu(x)
        self.relu_margin = margin
        return torch.tanh(x) * self.cfg.resd_limit

    def sdf_feat(self, cpts):
        """base_network.py:78-87 + SphereSignedDistanceField.forward net_utils.py:1337-1352."""
        inp = positional_encoding(cpts, self.cfg.sdf_res)
        x = inp
        for l, (w, b) in enumerate(self.sdf):
            hilo = None
            if l == 4:
                x = torch.cat([x, inp], dim=-1)
                if self.emulate is None:
                    x = x / math.sqrt(2)
                else:
                    w = w / math.sqrt(2)         # the kernel folds 1/sqrt(2) into lin4's weights
                hilo = [x.shape[-1] - inp.shape[-1] + k for k in range(9)]
            elif l == 0:
                hilo = list(range(9))            # x, sin(x), cos(x)
            pe_cols = slice(x.shape[-1] - inp.shape[-1], x.shape[-1]) if l in (0, 4) else None
            x = self.lin(x, w, b, hilo_cols=hilo, scaled_x=l > 0, scaled_w_cols=pe_cols, seed=l == 8)
            if l < 8:
                x = self._softplus(x)
        return x[..., :1], x[..., 1:]

    def color_net(self, view, grad, feat, cond):
        """RenderNetwork.forward base_network.py:152-171."""
        net = torch.cat([positional_encoding(view, self.cfg.view_res), grad, feat], dim=-1)
        for i in range(3):
            net = F.relu(self.lin(net, *self.color[i]))
        net = torch.cat([net, cond.expand(net.shape[0], -1)], dim=-1)
        net = F.relu(self.lin(net, *self.color[3], exact_cols=slice(256, 256 + cond.shape[-1])))
        return torch.sigmoid(self.lin(net, *self.color[4]))

    def material(self, feat):
        """relight_network.py:45-47,97-98: 256->128->128->{3,1}, Softplus(100), slope*sigmoid+bias."""
        def run(layers, slope, bias):
            x = feat
            for i, (w, b) in enumerate(layers):
                x = self.lin(x, w, b)
                if i < len(layers) - 1:
                    x = softplus100(x)
            return slope * torch.sigmoid(x) + bias
        c = self.cfg
        return run(self.albedo, c.albedo_slope, c.albedo_bias), run(self.rough, c.roughness_slope, c.roughness_bias)


def _frame(batch):
    """squeeze the B=1 batch dim of the §8b frame-state keys."""
    f = odict()
    for k in ('R', 'Th', 'weights', 'A', 'big_A', 'pverts', 'pnorm', 'tverts', 'tnorm'):
        f[k] = batch[k][0].float()
    f.Th = f.Th.reshape(1, 3)
    f.cond = batch['poses'].reshape(1, -1).float()
    if 'train_motion' in batch:
        f.train_poses = batch['train_motion']['poses'][0].float()
    return f


def world_to_bigpose(net: OracleNet, x, fr, dist_th, v=None):
    """Network.world_to_bigpose base_network.py:238-336 (forward, transform, filtering)."""
    c = net.cfg
    ppts_all = (x - fr.Th) @ fr.R                                   # blend_utils.py:252-261
    sdf_batch, nn_batch, mask, d2, nn = geodesic_knn(ppts_all, fr.pverts, fr.pnorm, fr.tverts, c.sample_vert_cnt, dist_th,
                                                     use_geodesic_filter=c.get('use_geodesic_filter', True))
    ppts, d2, nn = ppts_all[mask], d2[mask], nn[mask]
    bw = fr.weights[nn]                                            # (S,K,J)  :287
    w = (-d2 / (2 * c.blend_radius ** 2)).exp()
    w = w / (w.sum(dim=-1, keepdim=True) + torch.finfo(w.dtype).eps)
    bw = (w[..., None] * bw).sum(dim=-2)                           # (S,J)
    big_A_bw = (bw[:, :, None, None] * fr.big_A[None]).sum(dim=1)  # blend_transform blend_utils.py:212-218
    big_R_inv = inverse_3x3(big_A_bw[:, :3, :3])
    A_bw = (bw[:, :, None, None] * fr.A[None]).sum(dim=1)
    R_inv = inverse_3x3(A_bw[:, :3, :3])
    tpts = torch.sum(R_inv * (ppts - A_bw[:, :3, 3])[:, None, :], dim=-1)          # :290-300
    bpts = torch.sum(big_A_bw[:, :3, :3] * tpts[:, None, :], dim=-1) + big_A_bw[:, :3, 3]   # :303-313
    ret = odict(tpts=tpts, bpts=bpts, d2=d2, nn=nn, mask=mask, nn_batch=nn_batch, sdf_batch=sdf_batch,
                A_bw=A_bw, R_inv=R_inv, big_A_bw=big_A_bw, big_R_inv=big_R_inv, ppts=ppts)
    if v is not None:
        pvds = (v @ fr.R)[mask]                                     # world_dirs_to_pose_dirs :225-231
        tvds = torch.sum(A_bw[:, :3, :3].mT * pvds[:, None, :], dim=-1)            # pose_dirs_to_tpose_dirs :276-287
        bvds = torch.sum(big_R_inv.mT * tvds[:, None, :], dim=-1)                 # tpose_dirs_to_pose_dirs :316-329
        ret.pvds, ret.tvds, ret.bvds = pvds, tvds, bvds
    return ret


def hdq_sdf(net: OracleNet, x, fr, dist_th=None, smooth_transition=True, return_parts=False):
    """Network.inference_world_distance_field base_network.py:365-387 (HDQ). x (P,3) -> (P,1)."""
    dist_th = net.cfg.dist_th if dist_th is None else dist_th
    ret = world_to_bigpose(net, x, fr, dist_th)
    cpts = ret.bpts + net.residuals(ret.bpts, fr.cond)
    net_sdf = net.sdf_feat(cpts)[0]
    smpl_sdf = ret.sdf_batch.mean(dim=-1, keepdim=True)
    smpl_sdf = torch.where(smpl_sdf < -dist_th, smpl_sdf, smpl_sdf.abs())
    if smooth_transition:
        d1 = smpl_sdf[ret.mask]
        r = (net_sdf.abs() / dist_th).clip(0, 1)
        net_sdf = d1 * r + net_sdf * (1 - r)
    sdf = smpl_sdf.clone()
    sdf[ret.mask] = net_sdf
    if return_parts:
        ret.sdf = sdf
        ret.smpl_sdf = smpl_sdf
        return ret
    return sdf


def observed_sdf(net: OracleNet, x, fr, smooth_transition=False, filtering=False, dist_th=None):
    """Network.inference_observed_distance_field base_network.py:389-449 (cfg.smpl_distance False): x are big-pose points;
    sdf = SDF(x + resd(x)); with filtering the hierarchical blend against the TEMPLATE body (geodesic_knn on tverts / tnorm)."""
    dist_th = net.cfg.dist_th if dist_th is None else dist_th
    sdf = net.sdf_feat(x + net.residuals(x, fr.cond))[0]
    if not filtering:
        return sdf
    sdf_batch, _, mask, _, _ = geodesic_knn(x, fr.tverts, fr.tnorm, fr.tverts, net.cfg.sample_vert_cnt, dist_th)
    smpl_sdf = sdf_batch.mean(dim=-1, keepdim=True)
    smpl_sdf = torch.where(smpl_sdf < -dist_th, smpl_sdf, smpl_sdf.abs())
    net_sdf = sdf[mask]
    if smooth_transition:
        r = (net_sdf.abs() / dist_th).clip(0, 1)
        net_sdf = smpl_sdf[mask] * r + net_sdf * (1 - r)
    out = smpl_sdf.clone()
    out[mask] = net_sdf
    return out


def affine_inverse(A):
    """blend_utils.py:11-15: transposes the 3x3 block (exact only for rigid transforms) and keeps the last row."""
    R, T, P = A[..., :3, :3], A[..., :3, 3:], A[..., 3:, :]
    return torch.cat([torch.cat([R.mT, -R.mT @ T], dim=-1), P], dim=-2)


def bigpose_transform(net: OracleNet, x, fr, backward=False, invert=False):
    """Network.world_to_bigpose_transform / bigpose_to_world_transform base_network.py:338-363: blended bone transforms of
    every point's 3 nearest vertices (transform=False -> no distance filtering, dist = 1e9), composed with the frame's R, Th."""
    c = net.cfg
    if backward:
        ppts, verts, norm = x, fr.tverts, fr.tnorm
    else:
        ppts, verts, norm = (x - fr.Th) @ fr.R, fr.pverts, fr.pnorm
    _, _, _, d2, nn = geodesic_knn(ppts, verts, norm, fr.tverts, c.sample_vert_cnt, 1e9)
    w = (-d2 / (2 * c.blend_radius ** 2)).exp()
    w = w / (w.sum(dim=-1, keepdim=True) + torch.finfo(w.dtype).eps)
    bw = (w[..., None] * fr.weights[nn]).sum(dim=-2)
    A_bw = (bw[:, :, None, None] * fr.A[None]).sum(dim=1)
    big_A_bw = (bw[:, :, None, None] * fr.big_A[None]).sum(dim=1)
    p2w = torch.eye(4)
    p2w[:3, :3], p2w[:3, 3] = fr.R, fr.Th.reshape(3)
    w2b = big_A_bw @ affine_inverse(A_bw) @ affine_inverse(p2w)[None]
    return affine_inverse(w2b) if invert else w2b


def bigpose_query(net: OracleNet, bpts, cond):
    """the geometry networks on big-pose points (inside forward_geometry, base_network.py:456-494; take_gradient net_utils.py:1215-1239):
    bpts, resd, cpts, sdf, feat and ograd = d sdf / d bpts (un-normalised; the HIP debug_full hook's `grad`), all detached"""
    bpts = bpts.detach().requires_grad_(True)
    with torch.enable_grad():
        resd = net.residuals(bpts, cond)
        cpts = bpts + resd
        sdf, feat = net.sdf_feat(cpts)
        ograd = torch.autograd.grad(sdf, bpts, torch.ones_like(sdf))[0]
    return bpts.detach(), resd.detach(), cpts.detach(), sdf.detach(), feat.detach(), ograd.detach()


def forward_geometry(net: OracleNet, x, v, fr, dist_th=None):
    """Network.forward_geometry base_network.py:456-494 (eval). Normals via autograd (net_utils.py:1215-1239)."""
    dist_th = net.cfg.dist_th if dist_th is None else dist_th
    out = world_to_bigpose(net, x, fr, dist_th, v)
    bpts, resd, cpts, sdf, feat, ograd = bigpose_query(net, out.bpts, fr.cond)
    occ = sdf_to_occ(sdf, net.beta)
    norm = normalize(ograd)
    norm = torch.sum(out.big_A_bw[:, :3, :3].mT * norm[:, None, :], dim=-1)   # pose_dirs_to_tpose_dirs(big)
    norm = torch.sum(out.R_inv.mT * norm[:, None, :], dim=-1)                 # tpose_dirs_to_pose_dirs(A)
    norm = norm @ fr.R.mT                                                     # pose_dirs_to_world_dirs
    norm = normalize(norm)
    out.bpts, out.cpts, out.resd = bpts, cpts, resd
    out.sdf, out.occ, out.feat, out.norm, out.ograd = sdf, occ, feat, norm, ograd
    return out


def network_forward(net: OracleNet, x, v, fr, dist_th=None):
    """eval-mode Network.forward: relight (relight_network.py:91-104) -> raw 17 ch
    [cpts,bpts,resd,albedo,roughness,norm,occ]; AniSDF (base_network.py:496-515) -> raw 16 ch
    [cpts,bpts,resd,norm,rgb,occ].  Zeros for points outside dist_th."""
    c = net.cfg
    if net.relight:
        out = forward_geometry(net, x, None, fr, dist_th)
        albedo, rough = net.material(out.feat)
        raw = torch.cat([out.cpts, out.bpts, out.resd, albedo, rough, out.norm, out.occ], dim=-1)
    else:
        out = forward_geometry(net, x, v, fr, dist_th)
        cond = fr.cond
        if c.fix_material >= 0 or c.always_fix_material:
            cond = fr.train_poses[c.fix_material].reshape(1, -1)    # base_network.py:501-503
        rgb = net.color_net(out.bvds, out.norm, out.feat, cond)
        raw = torch.cat([out.cpts, out.bpts, out.resd, out.norm, rgb, out.occ], dim=-1)
    full = raw.new_zeros(x.shape[0], raw.shape[-1])
    full[out.mask] = raw
    return full, out


# ----------------------------------------------------------------------------- tracing

def sphere_tracing(ray_o, ray_d, near, far, sdf_fn: Callable, iter=16, tan_i=1000.0, relax=0.0, offset=0.02,
                   eps=1e-8, shadow_skip_iter=1, clay_book=True, soft_shadow=False, tan_i_multiplier=1.0,
                   hard_tan_i=1000.0):
    """sphere_tracing sphere_tracing_renderer.py:103-216 (mode 'hdq'). near/far/tan_i (P,1) or scalars."""
    P = ray_o.shape[0]
    tan_i = hard_tan_i if not soft_shadow else tan_i_multiplier * tan_i
    ones = torch.ones(P, 1)
    near = ones * near
    far = ones * far
    tan = ones / tan_i
    off = ones * offset
    rlx = ones * relax
    occ = ones
    d0 = ones * 1e9
    d1 = ones * 1e9
    cd = ones * 1e9
    dt = ones * 1e9
    st = far
    ot = far
    t = near
    for i in range(iter):
        d1 = sdf_fn(ray_o + t * ray_d)
        if soft_shadow and clay_book and i >= shadow_skip_iter:
            dx0 = d0 + rlx * d0 + off
            dx1 = d1 + rlx * d1 + off
            dy = (dx1 ** 2) / (2 * dx0)
            dx = ((dx1 ** 2 - dy ** 2).sqrt() - off) / (1 + rlx)
            cls = dx.clip(0) / (t - dy).clip(near).clip(eps) / (tan * 2)
            msk = (cls < occ) & (dy < t) & (dx1 > 0) & (dx0 > 0) & (dx > 0) & (dy > 0) & (dy < dx0)
            ot = torch.where(msk, t - dy, ot)
            occ = torch.where(msk, cls, occ)
        if i >= shadow_skip_iter:
            cls = d1.clip(0) / t.clip(near).clip(eps) / (tan * 2)
            msk = cls < occ
            ot = torch.where(msk, t, ot)
            occ = torch.where(msk, cls, occ)
        if not soft_shadow:
            d1u, d0u = d1.abs(), d0.abs()
            msk = d0.sign() != d1.sign()
            st = torch.where(msk, t - dt * (d1u / (d0u + d1u + eps)).clip(0, 1), st)
            off = torch.where(msk, 0.0, off)
            rlx = torch.where(msk, 0.0, rlx)
            msk = d1u < cd
            cd = torch.where(msk, d1u, cd)
            st = torch.where(msk, t, st)
        dt = d1 + rlx * d1 + off
        t = t + dt
        t = torch.minimum(t, far)
        t = torch.maximum(t, near)
        d0 = d1
    return ray_o + st * ray_d, ray_o + ot * ray_d, occ, st, ot


def surface_trace(net: OracleNet, batch, noise: float = 0.0, generator=None):
    """the surface trace of render_human (sphere_tracing_renderer.py:571) alone, over all rays of `batch`; `noise`: std of a
    gaussian perturbation added to every distance the trace reads (fp32_unstable_rays).  Returns st, occ (P)."""
    c = net.cfg
    fr = _frame(batch)
    ray_o, ray_d, near, far = (batch[k][0].float() for k in ('ray_o', 'ray_d', 'near', 'far'))

    def fn(x):
        d = hdq_sdf(net, x, fr, c.dist_th, True)
        return d if noise == 0.0 else d + noise * torch.randn(d.shape, generator=generator)
    st_cfg = c.sphere_tracing
    _, _, occ, st, _ = sphere_tracing(ray_o, ray_d, near[:, None], far[:, None], fn, iter=st_cfg.iter, relax=st_cfg.relax, offset=st_cfg.offset,
                                      eps=st_cfg.eps, shadow_skip_iter=st_cfg.shadow_skip_iter, clay_book=not c.no_claybook, soft_shadow=False,
                                      hard_tan_i=st_cfg.tan_i)
    return st[:, 0], occ[:, 0]


def fp32_unstable_rays(net: OracleNet, batch, trials: int = 32, noise: float = 3e-7, tol: float = 1e-4, seed: int = 0):
    """Rays whose traced surface the reference's OWN arithmetic does not pin: the fixed-iteration sphere trace
    (sphere_tracing_renderer.py:144-205) ends in a limit cycle on part of the rays, and its closest-approach rule `abs(d1) < cd -> st = t`
    (:194-197) then compares the distances of successive visits of the same phase — values that agree to ~1e-7 — so which visit wins,
    and with it a jump of `st` by millimetres, is decided by the last bits of fp32 sums (the BLAS' summation order).  A ray is reported
    when a gaussian perturbation of `noise` (fp32 rounding level: the oracle itself is 1.2e-7 rms from a float64 evaluation of the MLPs)
    on the distances moves its `st` by more than `tol`, or flips its hit status, in any of `trials` runs.  Returns a bool mask (P)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        st0, occ0 = surface_trace(net, batch)
        bad = torch.zeros_like(st0, dtype=torch.bool)
        for _ in range(trials):
            st, occ = surface_trace(net, batch, noise, g)
            bad |= ((st - st0).abs() > tol) | ((occ < 1) != (occ0 < 1))
    return bad


def fp32_flip_probability(net: OracleNet, batch, rays, noise: float, trials: int = 64, tol: float = 1e-4, seed: int = 1):
    """For the listed rays of `batch`: the fraction of `trials` runs in which gaussian noise of `noise` on the distances the surface trace
    reads moves `st` by more than `tol` or flips the hit status (see fp32_unstable_rays).  The rays are traced on their own (rays are
    independent units).  Returns a list of floats."""
    if len(rays) == 0:
        return []
    sub = type(batch)(batch)
    idx = torch.as_tensor(list(rays), dtype=torch.long)
    for k in ('ray_o', 'ray_d', 'near', 'far'):
        sub[k] = batch[k][:, idx].contiguous()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        st0, occ0 = surface_trace(net, sub)
        flips = torch.zeros_like(st0)
        for _ in range(trials):
            st, occ = surface_trace(net, sub, noise, g)
            flips += (((st - st0).abs() > tol) | ((occ < 1) != (occ0 < 1))).float()
    return [float(v) / trials for v in flips.reshape(-1)]


def key_lights(net: OracleNet, probes, share: float, kmax: int = 48):
    """the lights that hold at least the fraction max(share, 4 / L) of a probe's power (radiance x solid angle, channel mean) under any of
    `probes` (each (H, W, 3)): the rule of the key-light tier (csrc/ra_trace.hip key_lights_kernel)"""
    d = normalize(net.light_xyz.reshape(-1, 3))
    area = net.light_area.reshape(-1)
    smax = torch.zeros(d.shape[0])
    for pr in probes:
        w = (sample_envmap_image(pr, d).mean(-1) * area).clamp_min(0)
        smax = torch.maximum(smax, w / w.sum())
    key = smax >= max(share, 4.0 / d.shape[0])
    if int(key.sum()) > kmax:          # the kmax lights with the largest share
        keep = torch.zeros_like(key)
        keep[torch.topk(torch.where(key, smax, torch.zeros_like(smax)), kmax).indices] = True
        key = keep
    return key


def light_visibility(net: OracleNet, surf, norm, acc, fr, bbox, lvis_cfg, sdf_fn_factory):
    """light_visibility sphere_tracing_renderer.py:265-344. surf,norm (P,3), acc (P) -> lvis, ldot (L,P)."""
    c = net.cfg
    xyz = net.light_xyz.reshape(-1, 3)
    sharp = net.light_sharp.reshape(-1)
    L, P = xyz.shape[0], surf.shape[0]
    ray_d_l = normalize(xyz)                                           # directional (quirk 10)
    ldot = ray_d_l @ norm.T                                            # (L,P)
    if c.no_visibility:
        return torch.ones_like(ldot), ldot
    if c.local_visibility:
        return (ldot > 0).float(), ldot
    lfrt = (ldot > 0) & (acc > 0)[None]
    li, pi = torch.nonzero(lfrt, as_tuple=True)
    ro, rd = surf[pi], ray_d_l[li]
    near_offset = lvis_cfg['near_offset']
    n, f = get_near_far_aabb(bbox, ro, rd)
    n, f = n.clip(near_offset), f.clip(near_offset)
    box = n < f
    lbox = torch.zeros_like(lfrt)
    lbox[li, pi] = box
    li, pi, ro, rd, n, f = li[box], pi[box], ro[box], rd[box], n[box], f[box]
    sdf_fn = sdf_fn_factory(lvis_cfg['dist_th'])
    _, _, occ, _, _ = sphere_tracing(ro, rd, n[:, None], f[:, None], sdf_fn, iter=lvis_cfg['iter'],
                                     tan_i=sharp[li][:, None], relax=lvis_cfg['relax'], offset=lvis_cfg['offset'],
                                     eps=c.sphere_tracing.eps, shadow_skip_iter=c.sphere_tracing.shadow_skip_iter,
                                     clay_book=not c.no_claybook, soft_shadow=not c.no_dfss,
                                     tan_i_multiplier=c.sphere_tracing.tan_i_multiplier, hard_tan_i=c.sphere_tracing.tan_i)
    lvis = torch.zeros_like(ldot)
    lvis[li, pi] = occ[:, 0]
    lvis = lvis * lbox + 1 * ~lbox
    lvis = lvis * lfrt + 0 * ~lfrt
    return lvis, ldot


def shade_pixels(net: OracleNet, probe, ray_o, surf, norm, albedo, rough, lvis, ldot, want_spec=False, main_pass=True):
    """Shading block sphere_tracing_renderer.py:715-755 / novel_light_sphere_tracing.py:21-66.
    probe (H,W,3); per-pixel tensors (P,*); lvis/ldot (L,P). Returns rgb (sRGB), shade, spec (or None)."""
    c = net.cfg
    xyz = net.light_xyz.reshape(-1, 3)
    area = net.light_area.reshape(-1)
    surf2light = normalize(xyz[:, None] - surf[None])                 # (L,P,3)
    surf2cam = normalize(ray_o - surf)
    light = sample_envmap_image(probe, surf2light)                    # (L,P,3)
    # (main_pass False: the novel-light re-shade, novel_light_sphere_tracing.py:21-66, which knows none of the debugging switches below)
    if main_pass and c.get('only_visibility', False):                 # :720-723 (debugging option): uniform cosine, one-channel light
        ldot = torch.ones_like(ldot)
        light = light.mean(dim=-1, keepdim=True)
    ones = torch.ones_like(ldot)
    shade = lvis[..., None] * ones[..., None] * area[:, None, None] * light
    p2l = surf2light.permute(1, 0, 2)
    brdf = microfacet_brdf(p2l, surf2cam, norm, albedo, rough, f0=c.fresnel_f0,
                           lambert_only=c.lambert_only, glossy_only=c.glossy_only).permute(1, 0, 2)
    rgb = (brdf * shade).sum(0)
    if c.tonemapping_rendering:
        rgb = linear2srgb(rgb)
    spec = None
    if want_spec:
        sb = microfacet_brdf(p2l, surf2cam, norm, torch.zeros_like(albedo), rough, f0=c.fresnel_f0,
                             lambert_only=c.lambert_only, glossy_only=c.glossy_only).permute(1, 0, 2)
        sl = 1 / (torch.abs(ones) + 1e-8)
        spec = (sb * (ones[..., None] * sl[..., None] * area[:, None, None] * light)).sum(0)
    shade_map = (lvis[..., None] * ldot[..., None] * area[:, None, None] * light).sum(0) * c.shading_albedo / math.pi
    eH = c.env_h                                                      # :756-757: mean over the probe's rows, then over its columns
    if main_pass and c.get('vis_lvis_map', False):
        shade_map = lvis.view(eH, -1, lvis.shape[-1]).mean(0).mean(0)[:, None].expand(-1, 3)
    if main_pass and c.get('vis_ldot_map', False):
        shade_map = ldot.view(eH, -1, ldot.shape[-1]).mean(0).mean(0)[:, None].expand(-1, 3)
    return rgb, shade_map, spec


# ----------------------------------------------------------------------------- renderers

def _chunks(total, chunk):
    """chunkify's size rule net_utils.py:323."""
    if total == 0:
        return [(0, 0)]
    actual = math.ceil(total / math.ceil(total / chunk))
    return [(i, min(i + actual, total)) for i in range(0, total, actual)]


def render_human(net: OracleNet, ray_o, ray_d, near, far, probe, fr, bbox):
    """render_human sphere_tracing_renderer.py:551-784, eval mode, one chunk. Returns full-ray maps."""
    c = net.cfg
    P = ray_o.shape[0]
    st_cfg = c.sphere_tracing
    surf_all, edge, occ, st, ot = sphere_tracing(
        ray_o, ray_d, near[:, None], far[:, None], lambda x: hdq_sdf(net, x, fr, c.dist_th, True),
        iter=st_cfg.iter, relax=st_cfg.relax, offset=st_cfg.offset, eps=st_cfg.eps,
        shadow_skip_iter=st_cfg.shadow_skip_iter, clay_book=not c.no_claybook, soft_shadow=False, hard_tan_i=st_cfg.tan_i)
    depth_all = (surf_all[:, 0] - ray_o[:, 0]) / ray_d[:, 0]          # quirk 4
    acc_all = 1 - occ[:, 0]
    hit = acc_all > 0
    acc, surf, view, ro, depth = acc_all[hit], surf_all[hit], ray_d[hit], ray_o[hit], depth_all[hit]
    S = c.n_samples
    zval = torch.full((1,), 0.5) if S == 1 else torch.linspace(0.0, 1.0, steps=S)
    net_zval = zval * (2 * c.surf_sample_range) - c.surf_sample_range
    net_view = view[:, None, :].expand(-1, S, -1)
    net_surf = surf[:, None, :] + net_zval[None, :, None] * net_view
    raw, _ = network_forward(net, net_surf.reshape(-1, 3), net_view.reshape(-1, 3), fr, c.dist_th)
    raw_samples = raw                                                 # ret.raw of net_decoder, (hits * S, C): returned as is (:616)
    raw = raw.view(surf.shape[0], S, -1)
    raw, o = raw[..., :-1], raw[..., -1]
    _, raw, o = volume_rendering(raw, o, bg_brightness=c.bg_brightness)
    raw = raw / (o[..., None] + 1e-8)
    ret = odict(acc_map=acc, ray_o=ro, surf_map=surf, depth_map=depth, raw=raw_samples)
    if net.relight:
        cpts, bpts, resd, albedo, rough, norm = raw.split([3, 3, 3, 3, 1, 3], dim=-1)
    else:
        cpts, bpts, resd, norm, rgb = raw.split([3, 3, 3, 3, 3], dim=-1)
    norm = torch.where(norm.sum(dim=-1, keepdim=True) == 0, torch.ones_like(norm), norm)
    norm = normalize(norm)
    ret.cpts_map, ret.bpts_map, ret.resd_map, ret.norm_map = cpts, bpts, resd, norm
    if net.relight:
        albedo = albedo.clip(c.albedo_bias, c.albedo_bias + c.albedo_slope)
        rough = rough.clip(c.roughness_bias, c.roughness_bias + c.roughness_slope)
        ret.volume_albedo, ret.volume_roughness = albedo, rough
        if c.albedo_multiplier > 0:
            albedo = albedo * c.albedo_multiplier
        ret.albedo_map, ret.roughness_map = albedo, rough[:, 0]
    # :702-705: with none of the rendering / shading / specular maps wanted, render_human returns before any shading (no rgb_map)
    early = not (c.get('vis_rendering_map', True) or c.get('vis_shading_map', False) or c.get('vis_specular_map', False))
    if early:
        pass
    elif c.relighting:
        snet = net.shadow_net or net                                   # tiered precision (tools/precision_tiers.py)
        lvis, ldot = light_visibility(net, surf, norm, acc, fr, bbox, c.obj_lvis,
                                      lambda th: (lambda x: hdq_sdf(snet, x, fr, th, True)))
        key = getattr(net, 'key_lights', None)                         # emulation of cfg.trace_precision's key-light tier: the rays towards
        if key is not None and snet is not net and bool(key.any()):    # the lights that carry the probe's power are traced by `net` itself
            lvis_k, _ = light_visibility(net, surf, norm, acc, fr, bbox, c.obj_lvis, lambda th: (lambda x: hdq_sdf(net, x, fr, th, True)))
            lvis = torch.where(key.reshape(-1, 1), lvis_k, lvis)
        rgb, shade, spec = shade_pixels(net, probe, ro, surf, norm, albedo, rough, lvis, ldot, want_spec=c.vis_specular_map)
        ret.rgb_map, ret.shade_map = rgb, shade
        if spec is not None:
            ret.spec_map = spec
        if c.vis_novel_light:
            ldot_kept = torch.ones_like(ldot) if c.get('only_visibility', False) else ldot          # :758-759: the cosines as the shading used them
            ret.lvis_map, ret.ldot_map = lvis.T.contiguous(), ldot_kept.T.contiguous()     # (P,512)
    else:
        ret.rgb_map = rgb
    full = odict()
    for k, vv in ret.items():
        if k in ('volume_albedo', 'volume_roughness', 'raw'):          # per-hit arrays: not scattered (not in expanding_keys, :662-677)
            full[k] = vv
            continue
        z = vv.new_zeros(P, *vv.shape[1:])
        z[hit] = vv
        full[k] = z
    full.hit = hit
    return full


BLEND_KEYS = ['rgb_map', 'rfl_map', 'surf_map', 'albedo_map', 'roughness_map', 'norm_map', 'cpts_map', 'bpts_map',
              'spec_map', 'depth_map', 'lvis_map', 'ldot_map', 'brdf_map', 'shade_map']


def rodrigues(rot_vecs: torch.Tensor):
    """batch_rodrigues, data_utils.py:1004-1023 (the numpy twin of smplx.lbs.batch_rodrigues): float64 inside, float32 out."""
    r = rot_vecs.double()
    angle = torch.linalg.norm(r + 1e-8, dim=1, keepdim=True)
    d = r / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    z = torch.zeros_like(rx)
    K = torch.cat([z, -rz, ry, rz, z, -rx, -ry, rx, z], dim=1).view(-1, 3, 3)
    return (torch.eye(3, dtype=torch.float64)[None] + sin * K + (1 - cos) * (K @ K)).float()


def rigid_transforms(poses, joints, parents):
    """get_rigid_transformation_and_joints, data_utils.py:1026-1069 (== smplx.lbs.batch_rigid_transform, which
    net_utils.py:1164-1183 calls): per-bone rest-to-posed 4x4 `A` and the posed joints.  poses, joints (J,3), parents (J)."""
    J = joints.shape[0]
    R = rodrigues(poses).double()
    jt = joints.double()
    rel = jt.clone()
    rel[1:] -= jt[parents[1:]]
    T = torch.zeros(J, 4, 4, dtype=torch.float64)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, rel, 1.0
    chain = [T[0]]
    for i in range(1, J):
        chain.append(chain[int(parents[i])] @ T[i])
    tr = torch.stack(chain)
    posed = tr[:, :3, 3].clone()
    jh = torch.cat([jt, torch.zeros(J, 1, dtype=torch.float64)], dim=1)
    tr[:, :, 3] = tr[:, :, 3] - (tr * jh[:, None]).sum(-1)
    return tr.float(), posed.float()


def verts_normals(verts, faces):
    """pytorch3d.structures.Meshes.verts_normals_packed (un-vendored dependency, version unpinned: PARITY UNPINNED — restated
    from its published algorithm): area-weighted face normals accumulated per corner with that corner's edge pair, then
    F.normalize(eps=1e-6)."""
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = torch.zeros_like(verts)
    n = n.index_add(0, faces[:, 1], torch.cross(v2 - v1, v0 - v1, dim=1))
    n = n.index_add(0, faces[:, 2], torch.cross(v0 - v2, v1 - v2, dim=1))
    n = n.index_add(0, faces[:, 0], torch.cross(v1 - v0, v2 - v0, dim=1))
    return F.normalize(n, eps=1e-6, dim=1)


def pose_frame(poses, tjoints, parents, tverts, weights, big_A, faces, Rh, Th, padding=0.05):
    """N3: base_dataset.py:308-397 (get_lbs_params with cfg.use_geometry, get_blend): bone transforms, template -> T pose ->
    posed -> world vertices (blend_utils.py:212-218,264-313), vertex normals, bounds (data_utils.py:616-622)."""
    A, Jp = rigid_transforms(poses, tjoints, parents)
    Abig = torch.einsum('nj,jab->nab', weights, big_A)
    t = tverts - Abig[:, :3, 3]
    txyz = (inverse_3x3(Abig[:, :3, :3]) * t[:, None]).sum(-1)
    Abw = torch.einsum('nj,jab->nab', weights, A)
    pxyz = (Abw[:, :3, :3] * txyz[:, None]).sum(-1) + Abw[:, :3, 3]
    R = rodrigues(Rh[None])[0]
    wxyz = pxyz @ R.mT + Th
    bnd = lambda x: torch.stack([x.min(0)[0] - padding, x.max(0)[0] + padding])
    return odict(A=A, joints=Jp, tverts=txyz, pverts=pxyz, wverts=wxyz, R=R, pnorm=verts_normals(pxyz, faces),
                 pbounds=bnd(pxyz), wbounds=bnd(wxyz))


def get_rays_torch(H, W, K, R, T):
    """get_rays net_utils.py:403-425 (torch, the camera's dtype): full-frame rays, (H*W,3) each."""
    ray_o = -(R.mT @ T).ravel()
    i, j = torch.meshgrid(torch.arange(H, dtype=R.dtype), torch.arange(W, dtype=R.dtype), indexing='ij')
    xy1 = torch.stack([j, i, torch.ones_like(i)], dim=2)
    pixel_camera = xy1 @ torch.inverse(K).mT
    pixel_world = (pixel_camera - T.ravel()) @ R
    ray_d = normalize(pixel_world - ray_o[None, None])
    return ray_o[None].expand(H * W, 3), ray_d.reshape(-1, 3)


def render_ground(net: OracleNet, ray_o, ray_d, acc, probe, fr, bbox):
    """render_ground sphere_tracing_renderer.py:463-548, one chunk: ray/plane hit (moller_trumbore on one triangle of the
    plane, mesh_utils.py:710-738 — its t reduces to -((o-orig).n)/(d.n + eps/|a|^2); the triangle's random edge only scales
    eps), DFSS shadows of the avatar onto the plane with cfg.env_lvis, Lambert ground lit by the probe, distance fade.
    ray_o, ray_d (P,3); acc (P) = 1 - human acc; returns per-pixel maps."""
    c = net.cfg
    n = normalize(torch.tensor(c.ground_normal, dtype=torch.float32))
    orig = torch.tensor(c.ground_origin, dtype=torch.float32)
    t = -((ray_o - orig) @ n) / ((ray_d @ n) + 1e-8)
    surf = ray_o + t[:, None] * ray_d
    norm = n[None].expand_as(surf)
    lvis, _ = light_visibility(net, surf, norm, acc, fr, bbox, c.env_lvis, lambda th: (lambda x: hdq_sdf(net, x, fr, th, True)))
    albedo = sample_envmap_image(probe, ray_d) if c.ground_attach_envmap else torch.tensor(c.ground_albedo)[None].expand_as(surf)
    dist = torch.where(t <= 0, torch.full_like(t, 1e9), (surf - orig).norm(dim=-1))
    weight = ((dist - c.env_r) / c.env_r).clip(0, 1)                       # (P)
    xyz = net.light_xyz.reshape(-1, 3)
    area = net.light_area.reshape(-1)
    ldir = normalize(xyz)
    ldot = (ldir @ n)[:, None].expand(-1, surf.shape[0])                   # (L,P): NOT clamped (:504)
    lvis = lvis * (1 - weight)[None] + weight[None]
    light = sample_envmap_image(probe, ldir)                               # (L,3)
    if c.get('only_visibility', False):                                    # :516-519 (debugging option): uniform cosine, one-channel light:
        ldot = torch.ones_like(ldot)                                       # shade / spec come out with ONE channel and broadcast in the blend
        light = light.mean(dim=-1, keepdim=True)
    shade = lvis[..., None] * ldot[..., None] * area[:, None, None] * light[:, None, :]
    rgb = ((albedo / math.pi)[None] * shade).sum(0)
    if c.tonemapping_rendering:
        rgb = linear2srgb(rgb)
    shade = shade.sum(0) * c.shading_albedo / math.pi
    shade_map = shade
    if c.get('vis_lvis_map', False):                                       # :537-538: mean over the probe's rows, then its columns
        shade_map = lvis.view(c.env_h, -1, lvis.shape[-1]).mean(0).mean(0)[:, None].expand(-1, 3)
    if c.get('vis_ldot_map', False):
        shade_map = ldot.reshape(c.env_h, -1, ldot.shape[-1]).mean(0).mean(0)[:, None].expand(-1, 3)
    ret = odict(rgb_map=rgb, surf_map=surf, albedo_map=albedo, roughness_map=torch.ones_like(t), spec_map=shade / 20,
                norm_map=norm, shade_map=shade_map * c.ground_shading_multiplier, cpts_map=torch.zeros_like(surf),
                bpts_map=torch.zeros_like(surf), depth_map=t.clip(-c.env_r, c.env_r))
    if c.vis_novel_light:                                                  # :541-543, (P,L) like the human layer's
        ret.lvis_map, ret.ldot_map = lvis.T.contiguous(), ldot.T.contiguous()
    return ret


def blend_output_(acc_g, inds, grd, ret):
    """blend_output_ + alpha_blend / alpha_times (sphere_tracing_renderer.py:396-451), un-batched maps: the human layer
    (P rows) is scattered to the F frame pixels through inds and mixed with the ground layer by acc_g = 1 - human acc."""
    for k in BLEND_KEYS:
        if k in ret and k in grd:
            sc = torch.zeros(grd[k].shape[0], *ret[k].shape[1:])
            sc[inds] = ret[k]
            ag = acc_g if grd[k].ndim == 1 else acc_g[:, None]
            ret[k] = grd[k] * ag + sc * (1 - ag)
        elif k in grd:
            ret[k] = grd[k] * (acc_g if grd[k].ndim == 1 else acc_g[:, None])
    sc = torch.zeros_like(acc_g)
    sc[inds] = ret.acc_map
    ret.acc_map = sc * (1 - acc_g)                                       # alpha_blend(acc, inds, zeros, acc_map) (:449)
    return ret


def render_sphere_tracing(net: OracleNet, batch, probe=None, mutate_bounds=True, ground_inds=None):
    """Renderer.render sphere_tracing_renderer.py:1066-1115 (no ground pass): chunk rays, grow bbox
    IN PLACE per chunk (quirk 1), render_human, premultiply by acc (alpha_output_ :454-460).
    Returns batched (1,P,...) maps like the reference."""
    c = net.cfg
    fr = _frame(batch)
    if probe is None and net.relight:
        probe = net.global_env_map
    ray_o, ray_d, near, far = (batch[k][0].float() for k in ('ray_o', 'ray_d', 'near', 'far'))
    wb = batch['wbounds'] if mutate_bounds else batch['wbounds'].clone()
    outs = []
    for (a, b) in _chunks(ray_o.shape[0], c.render_chunk_size):
        wb[:, 0] -= c.env_lvis.bbox_margin
        wb[:, 1] += c.env_lvis.bbox_margin
        outs.append(render_human(net, ray_o[a:b], ray_d[a:b], near[a:b], far[a:b], probe, fr, wb[0].float()))
    ret = odict()
    for k in outs[0]:
        ret[k] = torch.cat([o[k] for o in outs], dim=0)
    if c.vis_ground_shading:
        # Renderer.render :1084-1111: full-frame rays, acc = 1 - human acc scattered to the in-box pixels, ground chunks
        # (each growing batch.wbounds again: get_ground_value :1054-1056), then blend_output_ (:434-451)
        H, W = int(batch['meta']['H'][0]), int(batch['meta']['W'][0])
        # the reference takes the in-box pixel indices from batch_aware_indexing = topk(sorted=False) (net_utils.py:381-389),
        # whose order is implementation-defined (not ascending on CPU): `ground_inds` lets a test reproduce a given order
        inds = batch['mask_at_box'].reshape(-1).nonzero()[:, 0] if ground_inds is None else ground_inds
        g_o, g_d = get_rays_torch(H, W, batch['cam_K'][0], batch['cam_R'][0], batch['cam_T'][0])
        acc_g = torch.ones(H * W)
        acc_g[inds] = 1 - ret.acc_map
        gouts = []
        for (a, b) in _chunks(H * W, c.render_chunk_size):
            wb[:, 0] -= c.env_lvis.bbox_margin
            wb[:, 1] += c.env_lvis.bbox_margin
            gouts.append(render_ground(net, g_o[a:b].float(), g_d[a:b].float(), acc_g[a:b], probe, fr, wb[0].float()))
        grd = odict({k: torch.cat([o[k] for o in gouts], dim=0) for k in gouts[0]})
        grd.ray_o, grd.ray_d, grd.acc_map, grd.inds = g_o.float(), g_d.float(), acc_g, inds
        if c.vis_novel_light:                                             # :1106-1107: kept apart for the per-probe re-shade
            ret.ground = grd
            return odict({k: (v if k == 'ground' else v[None]) for k, v in ret.items()})
        ret = blend_output_(acc_g, inds, grd, ret)
        return odict({k: v[None] for k, v in ret.items()})
    acc = ret.acc_map
    for k in BLEND_KEYS:
        if k in ret:
            v = ret[k]
            ret[k] = v * (acc[:, None] if v.ndim == 2 else acc)
    return odict({k: v[None] for k, v in ret.items()})


def render_volume(net: OracleNet, batch):
    """base_renderer.Renderer.render base_renderer.py:115-129 + get_pixel_value :53-113 (eval)."""
    c = net.cfg
    fr = _frame(batch)
    ray_o, ray_d = batch['ray_o'][0].float(), batch['ray_d'][0].float()
    near = batch['near'][0].float().clip(min=c.clip_near)
    far = batch['far'][0].float().clip(max=c.clip_far)
    S = c.n_samples
    t_vals = torch.linspace(0.0, 1.0, steps=S)
    outs = []
    for (a, b) in _chunks(ray_o.shape[0], c.render_chunk_size):
        z_vals = near[a:b, None] * (1.0 - t_vals) + far[a:b, None] * t_vals
        pts = ray_o[a:b, None] + ray_d[a:b, None] * z_vals[..., None]
        P = pts.shape[0]
        view = ray_d[a:b, None].expand(-1, S, -1)
        raw, _ = network_forward(net, pts.reshape(-1, 3), view.reshape(-1, 3), fr, c.dist_th)
        raw = raw.view(P, S, -1)
        weights, raw_map, acc_map = volume_rendering(raw[..., :-1], raw[..., -1], bg_brightness=c.bg_brightness)
        depth = torch.sum(weights * z_vals, dim=-1)
        outs.append(odict(depth_map=depth, cpts_map=raw_map[:, 0:3], bpts_map=raw_map[:, 3:6], resd_map=raw_map[:, 6:9],
                          norm_map=raw_map[:, 9:12], rgb_map=raw_map[:, 12:15], acc_map=acc_map))
    return odict({k: torch.cat([o[k] for o in outs])[None] for k in outs[0]})


def reshade_ground(net: OracleNet, probe, ray_d, albedo_map, lvis, ldot, image=None):
    """novel_light_sphere_tracing.render_ground :70-99 for one probe: Lambert ground from the cached (L,P) visibility / cosine."""
    c = net.cfg
    xyz = net.light_xyz.reshape(-1, 3)
    area = net.light_area.reshape(-1)
    light = sample_envmap_image(probe, normalize(xyz))                     # (L,3): surf2light = normalize(xyz - 0)
    albedo = sample_envmap_image(probe if image is None else image, ray_d) if c.ground_attach_envmap else albedo_map
    shade = lvis[..., None] * ldot[..., None] * area[:, None, None] * light[:, None, :]
    rgb = linear2srgb(((albedo / math.pi)[None] * shade).sum(0))
    shade = shade.sum(0) / math.pi
    return rgb, albedo, shade, shade / 20


def render_novel_light(net: OracleNet, batch, ground_inds=None):
    """novel_light_sphere_tracing.Renderer.render :103-221.  Without cfg.vis_ground_shading the re-shading consumes maps
    already premultiplied by acc (quirk 9); with it (the README command) both layers stay un-premultiplied, each is re-shaded
    per probe and blend_output_ merges them per light (:191-213) and for 'main' (:160-161)."""
    c = net.cfg
    main = render_sphere_tracing(net, batch, ground_inds=ground_inds)
    grd = main.get('ground', None)
    relight = odict()
    visual = ['rgb_map', 'acc_map', 'norm_map', 'surf_map', 'bpts_map', 'cpts_map', 'spec_map', 'shade_map',
              'depth_map', 'albedo_map', 'roughness_map']
    if 'main' in c.test_light:
        relight.main = odict({k: main[k] for k in visual if k in main})
        if grd is not None:
            m = blend_output_(grd.acc_map, grd.inds, grd, odict({k: v[0] for k, v in relight.main.items()}))
            relight.main = odict({k: v[None] for k, v in m.items()})
    lights = batch['novel_lights']
    if c.get('vis_rotate_light', False) and len(lights):      # :163-171: every probe at rotate_ratio * env_w headings
        rot = odict()
        for i in range(len(lights) * c.rotate_ratio * c.env_w):
            name, probe, image = rotate_envmap(lights, i, c.rotate_ratio, c.env_w, with_image=True)
            rot[name] = odict(probe=probe[None], **({'image': image[None]} if image is not None else {}))
        lights = rot
    for name, env in lights.items():
        probe = env['probe'][0].float()
        rgbs, shades, specs = [], [], []
        P = main.ray_o.shape[1]
        for (a, b) in _chunks(P, c.render_chunk_size):
            rgb, shade, spec = shade_pixels(net, probe, main.ray_o[0, a:b], main.surf_map[0, a:b], main.norm_map[0, a:b],
                                            main.albedo_map[0, a:b], main.roughness_map[0, a:b, None],
                                            main.lvis_map[0, a:b].T, main.ldot_map[0, a:b].T, want_spec=True, main_pass=False)
            rgbs.append(rgb), shades.append(shade), specs.append(spec)
        human = odict(rgb_map=torch.cat(rgbs), shade_map=torch.cat(shades), spec_map=torch.cat(specs))
        if grd is not None:
            image = env['image'][0].float() if 'image' in env else None
            g_rgb, g_alb, g_shade, g_spec = reshade_ground(net, probe, grd.ray_d, grd.albedo_map, grd.lvis_map.T, grd.ldot_map.T, image)
            ground = odict({k: grd[k] for k in visual if k in grd})
            ground.update(rgb_map=g_rgb, albedo_map=g_alb, shade_map=g_shade, spec_map=g_spec)
            full = odict({k: main[k][0] for k in visual if k in main})
            full.update(human)
            human = blend_output_(grd.acc_map, grd.inds, ground, full)
        else:
            full = odict({k: main[k][0] for k in visual if k in main})          # human = dotdict({**main, **human}) (:188)
            full.update(human)
            human = full
        relight[name] = odict({k: v[None] for k, v in human.items()})
        relight[name].envmap = odict(probe=env['probe'])
    relight._main_full = main
    return relight


def generate_image(output, batch, kind: str, cfg):
    """Visualizer.generate_image lib/visualizers/base_visualizer.py:54-208 (no ground truth): kind is the Output member's name.
    output: batched maps (1,P,..); returns the (H,W,3|4) image as a tensor."""
    H, W = int(batch['meta']['H'][0]), int(batch['meta']['W'][0])
    acc = output['acc_map'][0]

    def kth(v, frac, numel):                      # "a simple version of percentile" (:108-109)
        k = int(frac * numel)
        v = v.ravel()
        return v.topk(k, largest=False)[0].max(), v.topk(k, largest=True)[0].min()
    if kind == 'Normal':
        n = normalize(output['norm_map'][0]) @ batch['cam_R'][0].mT
        n = n * torch.tensor([1.0, -1.0, -1.0])
        rgb = (n * 0.5 + 0.5) * acc[:, None]
    elif kind == 'Alpha':
        rgb = acc[:, None].expand(-1, 3)
    elif kind == 'Depth':
        d = output['depth_map'][0]
        lo, hi = kth(d[acc.bool()], 0.01, d.numel())
        lo = lo.clip(None, cfg.min_clip)
        rgb = ((d - lo) / (hi - lo)).clip(0, 1)[:, None].expand(-1, 3)
    elif kind in ('Shading', 'Specular'):
        rgb = output['shade_map' if kind == 'Shading' else 'spec_map'][0]
        if cfg.normalize_shading if kind == 'Shading' else cfg.normalize_specular:
            rgb = rgb / kth(rgb, 0.005, rgb.numel())[1]
    elif kind == 'Albedo':
        rgb = linear2srgb(output['albedo_map'][0]) if cfg.tonemapping_albedo else output['albedo_map'][0]
    elif kind == 'Roughness':
        rgb = output['roughness_map'][0][:, None].expand(-1, 3)
    elif kind == 'Surface':
        m = output['cpts_map'][0] if 'cpts_map' in output else output['surf_map'][0]
        tb = batch['tbounds'][0]
        rgb = acc[:, None] * ((m - tb[0:1]) / (tb[1:2] - tb[0:1]))
    elif kind == 'Residual':
        d = output['cpts_map'][0] - output['bpts_map'][0]
        rgb = acc[:, None] * (d / kth(d, 0.005, d.numel())[1])
    elif kind == 'Rendering':
        rgb = output['rgb_map'][0]
    else:
        raise NotImplementedError(kind)
    mask = batch['mask_at_box'][0].reshape(H, W)
    img = torch.ones(H, W, 3) * cfg.bg_brightness
    img[mask] = rgb
    if cfg.probe_size_ratio > 0 and output.get('envmap', None) is not None:
        img = add_light_probe(img.reshape(H * W, 3), output['envmap']['probe'][0], H, W, batch['cam_R'][0], cfg.env_h, cfg.env_w,
                              cfg.probe_size_ratio).reshape(H, W, 3)
    if cfg.store_alpha_channel:
        alpha = torch.zeros(H, W, 1)
        alpha[mask] = acc[:, None]
        img = torch.cat([img, alpha], dim=-1)
    return img


def psnr(a, b):
    """lib/evaluators/base_evaluator.py:26-29."""
    mse = torch.mean((a - b) ** 2)
    return float(-10 * torch.log10(mse)) if mse > 0 else float('inf')

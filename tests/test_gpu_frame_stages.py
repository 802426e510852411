"""Edge-shape parity of the frame set-up, image and compositing kernels (DESIGN.md "Edge-shape parity of the frame stages").
Run with `-m gpu` on an MI355X.

    a  bone_transforms / lbs_verts / vert_normals / bounds   Engine.pose_frame          test_body_state*, test_bounds_*, test_face_content_*
    b  ray_mask / ray_emit                                    Engine.gen_rays            test_ray_generation
    c  debug_aabb (aabb_near_far, the shadow-ray clip)        Engine.debug_aabb          test_aabb_clip
    d  mf_view / mf_light                                     Engine.debug_brdf          test_brdf
    e  shift_envmap / light_probe                             Engine.shift_envmap, .add_light_probe     test_shift_envmap, test_light_probe_inset
    f  compose + the hipcub percentile chain                  Visualizer.generate_image  test_image_*
    g  volume_samples / volume_composite                      the AniSDF volume renderer test_volume_*
    h  gather_shard_rays / scatter_rows / blend_ground_* / grow_bounds                   test_gather_rays, test_scatter_rows, test_blend_ground, test_grow_bounds

No tolerance is chosen here.  frame_stage_ref.parity is DESIGN.md section 10's rule: per output, the kernel's max and median |diff| against the
float64 reference, normalised by max |ref|, at most 10 x the float32 reference's own error against float64 on the same inputs (computed
here, per case); where that error is exactly 0 the floor is 10 * 2^-23 * max |ref|; outputs without arithmetic (gathers, scatters, min / max,
selection order) are bit-equal.  The volume path runs the MLP on f16 operands: it is held to test_volume_switch_matrix's thresholds instead.
Every case prints kernel error, float32 error and ratio.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_stage_ref as R
from oracle import ra_oracle as O
from relightableavatar_amd import synthetic
from relightableavatar_amd._lib import RaError
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F32, F64 = torch.float32, torch.float64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _engine(mode='relight', **kw):
    from relightableavatar_amd.networks import make_network
    dev = _dev()
    cfg = make_cfg(mode, mlp_dtype='f16', **kw)
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=mode == 'relight', cfg=cfg))
    net = net.to(dev).eval()
    return cfg, net, dev, net.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))


@pytest.fixture(scope='module')
def relight():
    return _engine('relight')


def _pose(eng, c, dev, faces=None):
    return eng.pose_frame(c.poses, c.tjoints, c.parents, T(c.tverts).to(dev), T(c.weights).to(dev), c.big_A, c.faces if faces is None else faces,
                          c.Rh, c.Th, padding=c.padding)


def _own_bounds(verts, padding):
    """min / max -+ padding of the device's own float32 vertices, in float32"""
    v = verts.cpu()
    return torch.stack([v.min(0)[0] - np.float32(padding), v.max(0)[0] + np.float32(padding)])


# ------------------------------------------------------------------------------------------------ a. body state
@pytest.mark.parametrize('name', list(R.BODY_CASES))
def test_body_state(relight, name):
    """ra_pose_frame at J = 1 .. 256 (one lane loop, two, the API limit = 64 KB of LDS), chain / star / random trees, zero .. > 2 pi poses,
    the Rh = 0 identity branch, vertex counts around the 256- and 1024-thread strides, one-hot / uniform / 4-sparse weights, identity and
    real big poses, closed / isolated-vertex / zero-area / high-valence / odd-3F meshes"""
    _, _, dev, eng = relight
    c = R.body_case(name)
    o = _pose(eng, c, dev)
    r32, r64 = R.pose_frame(c, F32, c.padding), R.pose_frame(c, F64, c.padding)
    for k in ('A', 'joints', 'R', 'tverts', 'pverts', 'wverts', 'pnorm'):
        R.parity(f'body {name} {k}', o[k], r32[k], r64[k])
    # min / max involve no arithmetic: bit-equal to the bounds of the device's own vertices
    assert torch.equal(o.pbounds.cpu(), _own_bounds(o.pverts, c.padding)) and torch.equal(o.wbounds.cpu(), _own_bounds(o.wverts, c.padding))
    val = np.bincount(c.faces.reshape(-1), minlength=len(c.tverts))
    if (val == 0).any():
        assert float(o.pnorm.cpu()[T(val == 0)].abs().max()) == 0.0          # a vertex without a face: exactly 0
    if not c.Rh.any():
        assert torch.equal(o.R.cpu(), torch.eye(3))
    o2 = _pose(eng, c, dev)
    for k in ('A', 'joints', 'R', 'tverts', 'pverts', 'wverts', 'pnorm', 'pbounds', 'wbounds'):
        assert torch.equal(o[k], o2[k]), k                                     # two identical calls are bit-identical


def test_body_state_rejects_257_joints(relight):
    _, _, dev, eng = relight
    c = R.body_case('j256_n257_random')
    big = lambda a: np.concatenate([a, a[-1:]])
    with pytest.raises(RaError):
        eng.pose_frame(big(c.poses), big(c.tjoints), np.concatenate([c.parents, [0]]), T(c.tverts).to(dev),
                       T(np.concatenate([c.weights, np.zeros((len(c.tverts), 1), np.float32)], 1)).to(dev), big(c.big_A), c.faces, c.Rh, c.Th)


@pytest.mark.parametrize('padding', [0.0, 0.05])
@pytest.mark.parametrize('where', ['first', 'last', 'stride'])
def test_bounds_see_the_extreme_vertex(relight, where, padding):
    """the extreme vertex at index 0, at N - 1 and at an index = 1023 (mod 1024), the last thread of the one-workgroup reduction"""
    _, _, dev, eng = relight
    c = R.body_case('j2_n255')
    r = np.random.default_rng(3)
    N = 2050
    idx = {'first': 0, 'last': N - 1, 'stride': 2047}[where]
    c.tverts = r.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    c.tverts[idx] = [5.0, -6.0, 7.0]
    c.weights = R.make_weights(N, 2, 'onehot', r)
    c.faces = np.array([[0, 1, 2]])
    c.padding = padding
    o = _pose(eng, c, dev)
    pb, wb = _own_bounds(o.pverts, padding), _own_bounds(o.wverts, padding)
    assert torch.equal(o.pbounds.cpu(), pb) and torch.equal(o.wbounds.cpu(), wb)
    assert float(pb[1, 0]) == pytest.approx(5.0 + padding, abs=1e-4) and float(pb[0, 1]) == pytest.approx(-6.0 - padding, abs=1e-4)
    r64 = R.pose_frame(c, F64, padding)
    assert float((o.pbounds.cpu().double() - r64.pbounds).abs().max()) < 1e-5 and float((o.wbounds.cpu().double() - r64.wbounds).abs().max()) < 1e-5


def test_face_content_keys_the_adjacency_cache(relight):
    """two face arrays of equal F and N that differ in one index, posed one after the other on the same engine: the second call's normals
    follow the second array (the cached adjacency is keyed by the faces' content)"""
    _, _, dev, eng = relight
    c = R.body_case('j24_n256_isolated')
    c.tverts, f1, f2 = R.face_pair(256)
    refs = {}
    for tag, f in (('first', f1), ('second', f2), ('first again', f1)):
        c.faces = f
        o = _pose(eng, c, dev)
        r32, r64 = R.pose_frame(c, F32, c.padding), R.pose_frame(c, F64, c.padding)
        R.parity(f'face content, {tag} array: pnorm', o.pnorm, r32.pnorm, r64.pnorm)
        refs[tag] = o.pnorm.clone()
    assert not torch.equal(refs['first'], refs['second']) and torch.equal(refs['first'], refs['first again'])


# ------------------------------------------------------------------------------------------------ b. ray generation
@pytest.mark.parametrize('case', R.RAY_CASES, ids=lambda c: f'{c[0]}x{c[1]}-{c[2]}-{c[3]}')
def test_ray_generation(relight, case):
    """ra_gen_rays at H != W, H * W no multiple of 256, 1 x 1; the camera inside the box, a box covering every pixel / one pixel / behind
    the camera / off the view; a camera whose centre column and row have a zero direction component (the +-1e-5 replacement branches)"""
    _, _, dev, eng = relight
    H, W, cam, box = case
    K, Rc, Tc, bounds = R.ray_case(*case)
    o = eng.gen_rays(H, W, K, Rc, Tc, bounds)
    r32, r64 = R.ray_frame(H, W, K, Rc, Tc, bounds, F32), R.ray_frame(H, W, K, Rc, Tc, bounds, F64)
    dec = R.decided(r64, bounds)
    mask = o.mask_at_box.reshape(-1).cpu()
    assert torch.equal(mask[dec], r64.mask[dec]), f'{int((mask[dec] != r64.mask[dec]).sum())} decided pixels differ'
    pix = mask.nonzero()[:, 0]                                                  # ascending: the rays must come in row-major order
    P = pix.shape[0]
    print(f'rays {case}: {P} of {H * W} pixels in the box, {int((~dec).sum())} undecided')
    assert o.ray_o.shape == (P, 3) and o.ray_d.shape == (P, 3) and o.near.shape == (P,) and o.far.shape == (P,)
    keep = dec[pix]
    for k in ('ray_o', 'ray_d', 'near', 'far'):
        R.parity(f'rays {case} {k}', o[k], r32[k][pix], r64[k][pix], keep=keep)
    if P > 1:        # row-major order: every ray is closer to its own pixel's direction than to any other in-box pixel's
        d = o.ray_d.cpu().double()
        ref = r64.ray_d[pix].double()
        assert torch.equal((d @ ref.T).argmax(1), torch.arange(P))


# ------------------------------------------------------------------------------------------------ c. AABB clip
@pytest.mark.parametrize('n', [1, 255, 257])
def test_aabb_clip(relight, n):
    """the shadow-ray clip with direction components at and around the ends of the quirk's interval (-1e-16, 1e-8), origins inside the
    box, on a face and outside; errors relative per element where |ref| > 1 (divisions by 1e-8 .. 1e-17 reach 1e16)"""
    _, _, dev, eng = relight
    o, d = R.aabb_case(n)
    near, far = eng.debug_aabb(o.to(dev), d.to(dev), R.AABB_BOX.reshape(-1).tolist())
    (n32, f32), (n64, f64) = R.aabb(o, d, F32), R.aabb(o, d, F64)
    R.parity(f'aabb n={n} near', near, n32, n64, relative=True)
    R.parity(f'aabb n={n} far', far, f32, f64, relative=True)


# ------------------------------------------------------------------------------------------------ d. BRDF
@pytest.fixture(scope='module')
def brdf_engines(relight):
    return {'default': relight[3], 'lambert_only': _engine('relight', lambert_only=True)[3], 'glossy_only': _engine('relight', glossy_only=True)[3]}


@pytest.mark.parametrize('switch', ['default', 'lambert_only', 'glossy_only'])
@pytest.mark.parametrize('size', R.BRDF_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_brdf(brdf_engines, size, switch):
    """mf_view / mf_light at grazing (v.n = 1e-4, 0) and back-facing views, l = v, l = -v (zero half vector), l in the tangent plane, a
    zero-length normal, roughness at the bounds, albedo 0 and 1, under the ablation switches"""
    dev = _dev()
    eng = brdf_engines[switch]
    L, N = size
    c = R.brdf_case(L, N)
    out = eng.debug_brdf(c.p2l.to(dev), c.p2c.to(dev), c.normal.to(dev), c.albedo.to(dev), c.rough.to(dev)).cpu()
    kw = {} if switch == 'default' else {switch: True}
    b32, b64 = R.brdf(c, F32, **kw), R.brdf(c, F64, **kw)
    keep = ~R.brdf_near_switch(c)
    assert bool(torch.isfinite(out).all())                                     # also on the pairs left out
    R.parity(f'brdf {L}x{N} {switch}', out, b32, b64, keep=keep[..., None].expand(-1, -1, 3))


# ------------------------------------------------------------------------------------------------ e. envmap
@pytest.mark.parametrize('shape', R.ENV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shift_envmap(relight, shape):
    """ra_shift_envmap at other widths / channel counts, fractional, negative and multi-turn shifts"""
    _, _, dev, eng = relight
    H, W, C_ = shape
    img = R.env_image(H, W, C_)
    for s in R.ENV_SHIFTS(W):
        out = eng.shift_envmap(img.to(dev), s)
        R.parity(f'shift_envmap {shape} shift {s:g}', out, R.shift_envmap(img, s), R.shift_envmap(img.double(), s))


@pytest.mark.parametrize('probe_hw', R.PROBE_SIZES, ids=lambda s: f'probe{s[0]}x{s[1]}')
def test_light_probe_inset(relight, probe_hw):
    """ra_add_light_probe with empty, 1 x 1, 1 x 2, ordinary and full-image insets, both signs of cam_R[5]; outside the inset the image
    is untouched bit for bit"""
    _, _, dev, eng = relight
    H, W = R.PROBE_IMAGE
    rgb = R.env_image(H, W, 3, seed=1).reshape(-1, 3)
    probe = R.env_image(*probe_hw, 3, seed=2)
    for cam in R.probe_cams():
        for (uH, uW) in R.PROBE_INSETS:
            out = eng.add_light_probe(rgb.to(dev), probe.to(dev), H, W, cam, uH, uW).cpu()
            inset = torch.zeros(H, W, dtype=torch.bool)
            inset[:uH, :uW] = True
            assert torch.equal(out.reshape(H, W, 3)[~inset], rgb.reshape(H, W, 3)[~inset])
            if uH * uW:
                r32, r64 = R.add_light_probe(rgb, probe, H, W, cam, uH, uW), R.add_light_probe(rgb.double(), probe, H, W, cam, uH, uW)
                sel = inset.reshape(-1)
                R.parity(f'light probe {probe_hw} inset {uH}x{uW} cam_R[5] {float(cam[1, 2]):+.2f}', out[sel], r32[sel], r64[sel])


# ------------------------------------------------------------------------------------------------ f. visualiser
def _image(eng, cfg, maps, kind, H, W, pix, tb, cam_R, dev):
    """Visualizer.generate_image on un-batched maps: the scatter goes through batch.mask_at_box"""
    from relightableavatar_amd import config
    from relightableavatar_amd.base_utils import dotdict
    from relightableavatar_amd.visualizers import Output, Visualizer
    config.set_active_cfg(cfg)
    mask = torch.zeros(H * W, dtype=torch.bool)
    mask[pix] = True
    batch = dotdict(meta=dotdict(H=torch.tensor([H]), W=torch.tensor([W])), cam_R=cam_R[None].to(dev), tbounds=tb[None].to(dev), mask_at_box=mask[None].to(dev))
    out = dotdict({k: v[None].to(dev) for k, v in maps.items()})
    return T(Visualizer.generate_image(out, batch, Output[kind], engine=eng))


def _image_parity(label, img, maps, kind, cfg, H, W, pix, tb, cam_R):
    """the rule of the issue: identical NaN pattern, then parity on the finite pixels; background pixels are bg_brightness, alpha 0"""
    r32, r64 = (R.generate_image(maps, kind, cfg, H, W, pix, cam_R=cam_R, tbounds=tb, dtype=dt) for dt in (F32, F64))
    assert img.shape == (H, W, 4)
    assert bool((img.isnan() == r64.isnan()).all()), f'{label}: NaN pattern differs ({int(img.isnan().sum())} vs {int(r64.isnan().sum())})'
    bgm = torch.ones(H * W, dtype=torch.bool)
    bgm[pix] = False
    flat = img.reshape(-1, 4)
    assert bool((flat[bgm][:, :3] == np.float32(cfg.bg_brightness)).all()) and bool((flat[bgm][:, 3] == 0).all())
    assert torch.equal(flat[pix][:, 3], maps['acc_map'])                       # the alpha plane is a scatter: bit-equal
    fin = torch.isfinite(r64[..., :3]) & torch.isfinite(r32[..., :3])
    if bool(fin.any()):
        R.parity(label, img[..., :3], r32[..., :3], r64[..., :3], keep=fin)


@pytest.fixture(scope='module')
def image_cfg():
    return make_cfg('relight', probe_size_ratio=0.0, normalize_shading=True, bg_brightness=0.25)       # a background that is neither 0 nor the alpha plane's fill


@pytest.mark.parametrize('P', R.IMAGE_P)
def test_image_depth_edges(relight, image_cfg, P):
    """Depth through ra_map_to_image at the steps of k = int(0.01 P), on a non-square image: fewer hits than k (the documented clamp), no
    hit, NaNs of both sign bits, +-inf, all-equal maps"""
    _, _, dev, eng = relight
    maps, H, W, pix, tb = R.image_case(P)
    cam = synthetic.tilted_cam_R()[0]
    for name, (d, a) in [('plain', (maps.depth_map, maps.acc_map))] + list(R.depth_variants(maps).items()):
        m = O.odict(maps)
        m.depth_map, m.acc_map = d, a
        img = _image(eng, image_cfg, m, 'Depth', H, W, pix, tb, cam, dev)
        _image_parity(f'image Depth P={P} {H}x{W} {name}', img, m, 'Depth', image_cfg, H, W, pix, tb, cam)


def test_image_depth_needs_100_rays(relight, image_cfg):
    _, _, dev, eng = relight
    maps, H, W, pix, tb = R.image_case(99)
    with pytest.raises(RaError, match='too few rays for the percentile'):
        _image(eng, image_cfg, maps, 'Depth', H, W, pix, tb, synthetic.tilted_cam_R()[0], dev)


@pytest.mark.parametrize('kind', R.KINDS)
def test_image_every_output_type(relight, image_cfg, kind):
    """every Output type once at P = 257 (one ray past a 256-thread block) on a non-square image"""
    _, _, dev, eng = relight
    maps, H, W, pix, tb = R.image_case(257)
    cam = synthetic.tilted_cam_R()[0]
    img = _image(eng, image_cfg, maps, kind, H, W, pix, tb, cam, dev)
    _image_parity(f'image {kind} P=257 {H}x{W}', img, maps, kind, image_cfg, H, W, pix, tb, cam)


@pytest.mark.parametrize('P', R.IMAGE_P)
def test_image_unordered_pixel_list(relight, image_cfg, P):
    """ra_map_to_image with a shuffled `pix` (and the maps shuffled with it) gives the image of the ordered list, bit for bit: the scatter
    and the percentile selection do not depend on the order of the rays.  Depth at every P; Residual and Rendering at P = 257."""
    from relightableavatar_amd._lib import check, ra_image_params
    from relightableavatar_amd.visualizers import Output
    _, _, dev, eng = relight
    maps, H, W, pix, tb = R.image_case(P)
    cam = synthetic.tilted_cam_R()[0]
    perm = T(np.random.default_rng(9 + P).permutation(P))
    assert not bool((pix[perm][1:] > pix[perm][:-1]).all())
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for kind in ('Depth', 'Residual', 'Rendering') if P == 257 else ('Depth',):
        ordered = _image(eng, image_cfg, maps, kind, H, W, pix, tb, cam, dev)
        p = ra_image_params(type=Output[kind].value, H=H, W=W, bg_brightness=float(image_cfg.bg_brightness), normalize=1, tonemap=1,
                            min_clip=float(image_cfg.min_clip))
        a = {'Depth': maps.depth_map, 'Residual': maps.cpts_map, 'Rendering': maps.rgb_map}[kind][perm].contiguous().to(dev)
        b = maps.bpts_map[perm].contiguous().to(dev) if kind == 'Residual' else None
        acc, px = maps.acc_map[perm].contiguous().to(dev), pix[perm].contiguous().to(dev)
        image, alpha = torch.empty(H * W, 3, device=dev), torch.empty(H * W, device=dev)
        check(eng.lib.ra_map_to_image(eng.ctx, C.byref(p), ptr(a), ptr(b), ptr(acc), ptr(px), P, ptr(image), ptr(alpha), eng.stream), 'ra_map_to_image')
        got = torch.cat([image, alpha[:, None]], 1).reshape(H, W, 4).cpu()
        assert torch.equal(got, ordered), kind


# ------------------------------------------------------------------------------------------------ g. volume path
VOLUME_TOL = (('acc_map', 5e-4), ('depth_map', 1e-3), ('cpts_map', 2e-4), ('resd_map', 1e-5), ('norm_map', 2e-3), ('rgb_map', 3e-4))     # test_volume_switch_matrix


@pytest.fixture(scope='module')
def volume_rays():
    """65 in-box rays of a small frame (more than one 64-ray group)"""
    b = synthetic.make_batch(48, 48, seed=0, posed=True, crop=16, skin_noise=0.0)
    b, P, stride = synthetic.sample_rays(b, 70)
    assert b.ray_o.shape[1] >= 65, b.ray_o.shape
    # the ray that sees most of the body goes first (P = 1 must not be a miss); hits and misses follow in image order
    cfg = make_cfg('anisdf', n_samples=17, mlp_dtype='f16')
    acc = O.render_volume(O.OracleNet(synthetic.make_state_dict(0, relight=False, cfg=cfg), cfg), b).acc_map[0]
    first = int(acc.argmax())
    order = torch.tensor([first] + [i for i in range(acc.shape[0]) if i != first])
    for k in ('ray_o', 'ray_d', 'near', 'far'):
        b[k] = b[k][:, order].contiguous()
    assert float(acc[first]) > 0.3 and bool((acc[order[:63]] == 0).any()) and int((acc[order[:63]] > 0.05).sum()) > 20
    return b


def _volume_batch(rays, P):
    from relightableavatar_amd.base_utils import dotdict
    b = dotdict(rays)
    for k in ('ray_o', 'ray_d', 'near', 'far'):
        b[k] = rays[k][:, :P].contiguous()
    return b


def _render_volume(S, batch, dev, **kw):
    from relightableavatar_amd.networks import make_network
    from relightableavatar_amd.renderer import make_renderer
    cfg = make_cfg('anisdf', n_samples=S, mlp_dtype='f16', **kw)
    net = make_network(cfg)
    sd = synthetic.make_state_dict(0, relight=False, cfg=cfg)
    net.load_state_dict(sd)
    out = make_renderer(cfg, net.to(dev).eval()).render(synthetic.to_device(batch, dev))
    return cfg, sd, {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize('S,P', [(1, 65), (2, 65), (15, 65), (17, 65), (33, 65), (17, 1), (17, 63), (17, 64)])
def test_volume_ragged_segments(volume_rays, S, P):
    """ra_render_volume_chunk with sample counts that leave the 16 depth segments ragged or empty, and ray counts around the 64-ray group,
    against the oracle's render_volume on the same batch: test_volume_switch_matrix's keys and thresholds"""
    dev = _dev()
    batch = _volume_batch(volume_rays, P)
    cfg, sd, out = _render_volume(S, batch, dev)
    ref = O.render_volume(O.OracleNet(sd, cfg), batch)
    assert float(ref.acc_map.max()) > (0.3 if S >= 15 else 0.0)                # something is composited
    for k, tol in VOLUME_TOL:
        e = (out[k] - ref[k]).abs()
        print(f'volume S={S} P={P} {k}: max |diff| {float(e.max()):.2e} (threshold {tol:g})')
        assert out[k].shape == ref[k].shape and bool((e <= tol).all()), f'{k}: only {float((e <= tol).float().mean()) * 100:.1f}% of elements within {tol}'
    mse = float(((out['rgb_map'] - ref['rgb_map']) ** 2).mean())
    assert mse == 0 or -10 * np.log10(mse) > 80
    if S in (15, 17, 33) and P == 65:
        # the segments are summed in a fixed order: the maps do not depend on how the rays are chunked
        _, _, parts = _render_volume(S, batch, dev, render_chunk_size=24, volume_chunk_rays=0)
        for k, _ in VOLUME_TOL:
            assert torch.equal(parts[k], out[k]), f'{k}: chunks of 24 rays differ from one chunk'


# ------------------------------------------------------------------------------------------------ h. data movement
def _lib():
    from relightableavatar_amd import _lib
    return _lib


@pytest.mark.parametrize('n', [0, 1, 257])
def test_gather_rays(n):
    """ra_gather_rays (shard.shard_batch's binding) with repeated and reversed indices: torch indexing, bit for bit"""
    dev = _dev()
    L = _lib()
    r = np.random.default_rng(20 + n)
    P = 300
    src = [T(r.standard_normal(s).astype(np.float32)).to(dev) for s in ((P, 3), (P, 3), (P,), (P,))]
    idx = T(np.concatenate([np.arange(P)[::-1][:n // 2], r.integers(0, P, n - n // 2)]).astype(np.int64)).to(dev)
    if n > 2:
        idx[1] = idx[0]
    out = [torch.full((n,) + tuple(s.shape[1:]), -7.0, device=dev) for s in src]
    pt = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().ra_gather_rays(dev.index or 0, pt(idx), n, *[pt(t) for t in src], *[pt(t) for t in out],
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'ra_gather_rays')
    for o, s in zip(out, src):
        assert torch.equal(o, s[idx])


@pytest.mark.parametrize('C_', [1, 3, 24])
@pytest.mark.parametrize('n', [0, 1, 1000])
def test_scatter_rows(n, C_):
    """ra_scatter_rows (shard._unshuffle's binding): dst[dst_idx[i]] = src[src_idx[i]] with a permutation as dst_idx, bit for bit"""
    dev = _dev()
    L = _lib()
    r = np.random.default_rng(40 + n + C_)
    total = n + 5
    src = T(r.standard_normal((max(n, 1) + 3, C_)).astype(np.float32)).to(dev)
    dst_idx = T(r.permutation(total)[:n].astype(np.int64)).to(dev)
    src_idx = T(r.integers(0, src.shape[0], n).astype(np.int64)).to(dev)
    dst = torch.full((total, C_), -7.0, device=dev)
    ref = dst.clone()
    pt = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().ra_scatter_rows(dev.index or 0, pt(src), pt(src_idx), pt(dst_idx), n, C_, pt(dst),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'ra_scatter_rows')
    ref[dst_idx] = src[src_idx]
    assert torch.equal(dst, ref)


@pytest.mark.parametrize('C_', [1, 3])
def test_blend_ground(relight, C_):
    """Engine.blend_ground against blend_output_'s float32 arithmetic (one multiply and one multiply-add per pixel): with and without a
    ground layer (base 0), without rays (P = 0), `inds` a shuffled subset"""
    _, _, dev, eng = relight
    r = np.random.default_rng(60 + C_)
    F_, P = 777, 300
    f = lambda a: T(np.ascontiguousarray(a, dtype=np.float32))
    acc, grd, hum = f(r.uniform(0, 1, F_)), f(r.uniform(0, 2, (F_, C_))), f(r.uniform(0, 2, (P, C_)))
    inds = T(r.permutation(F_)[:P].astype(np.int64))
    shape = lambda t: None if t is None else (t[:, 0] if C_ == 1 else t)       # C = 1: the flat (F,) maps of the renderer
    for tag, g, h, ix in (('both', grd, hum, inds), ('ground=None', None, hum, inds), ('P=0', grd, hum[:0], inds[:0]), ('human=None', grd, None, inds[:0])):
        out = eng.blend_ground(None if g is None else shape(g).to(dev), None if h is None else shape(h).to(dev), ix.to(dev), acc.to(dev)).cpu()
        ref = R.blend_ground(g, h, ix, acc, F_, C_)
        d = lambda t: None if t is None else t.double()
        ref64 = (torch.zeros(F_, C_, dtype=F64) if g is None else d(g)) * acc.double()[:, None]
        if h is not None and h.shape[0]:
            sc = torch.zeros(F_, C_, dtype=F64)
            sc[ix] = d(h)
            ref64 = ref64 + sc * (1 - acc.double()[:, None])
        out = out.reshape(F_, C_)
        exact = bool(torch.equal(out, ref))
        print(f'blend_ground C={C_} {tag}: bit-equal to the float32 reference: {exact}')
        if not exact:       # a contracted multiply-add (one rounding instead of two): the rule's floor, not bit equality
            R.parity(f'blend_ground C={C_} {tag}', out, ref, ref64)
            assert float((out.double() - ref.double()).abs().max()) <= R.ULP * float(ref64.abs().max())


def test_grow_bounds(relight):
    """three successive growths of a (1,2,3) box equal torch's in-place float32 arithmetic, bit for bit"""
    _, _, dev, eng = relight
    wb = torch.tensor([[[-0.4123, -0.3377, -0.9051], [0.4519, 0.2873, 0.8807]]])
    dv = wb.clone().to(dev)
    for step in range(3):
        wb[:, 0] -= 0.05
        wb[:, 1] += 0.05
        eng.grow_bounds(dv, 0.05)
        assert torch.equal(dv.cpu(), wb), step

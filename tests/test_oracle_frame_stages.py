"""Pin tests/frame_stage_ref.py, the references test_gpu_frame_stages.py compares the kernels with.  CPU only.

Two things are asserted here, on the references alone:
  * run in float32 they reproduce the reference-made goldens (lbs.npz, rays.npz, envmap.npz, visual.npz, the aabb_* / mf_* entries of
    ops.npz) at the tolerances test_oracle_golden.py holds for the oracle, and agree with the oracle's own functions;
  * the conditions the GPU tests put on their INPUTS: at most 1 % of a frame's pixels have an undecided box mask, at most 2 % of a BRDF
    case's pairs sit near a step function, the blended big-pose 3 x 3 of every body case has |det| >= 0.1.
"""
import numpy as np
import pytest
import torch

import frame_stage_ref as R
from oracle import ra_oracle as O
from relightableavatar_amd import synthetic
from relightableavatar_amd.config import make_cfg

T = torch.from_numpy
F32, F64 = torch.float32, torch.float64


def maxdiff(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


# ------------------------------------------------------------------------------------------------ a. body state
def _golden_body():
    sk = synthetic.make_skeleton(0)
    big_A = R.rigid_transforms64(T(sk.big_poses), T(sk.tjoints), T(sk.parents))[0].float().numpy()
    return O.odict(poses=sk.poses, tjoints=sk.tjoints, parents=sk.parents, tverts=sk.tverts, weights=sk.weights, big_A=big_A, faces=sk.faces,
                   Rh=sk.Rh, Th=sk.Th)


def test_pose_frame_reference_reproduces_the_golden(golden):
    g = golden('lbs.npz')
    c = _golden_body()
    assert maxdiff(c.big_A, g['big_A']) < 1e-6
    o = R.pose_frame(c, F32)
    sel = T(g['sel'])
    assert maxdiff(o.A, g['A']) < 1e-6 and maxdiff(o.joints, g['joints']) < 1e-6 and maxdiff(o.R, g['R']) < 1e-6
    assert maxdiff(o.tverts[sel], g['txyz']) < 2e-6 and maxdiff(o.pverts[sel], g['pxyz']) < 2e-6 and maxdiff(o.wverts[sel], g['wxyz']) < 2e-6
    assert bool((o.pbounds[0] <= T(g['pbounds'])[0] + 1e-6).all()) and bool((o.pbounds[1] >= T(g['pbounds'])[1] - 1e-6).all())
    # ... and the oracle's pose_frame (its global rotation adds 1e-8 to the angle like batch_rodrigues; cv2.Rodrigues does not)
    ref = O.pose_frame(T(c.poses), T(c.tjoints), T(c.parents), T(c.tverts), T(c.weights), T(c.big_A), T(c.faces), T(c.Rh), T(c.Th))
    assert torch.equal(o.A, ref.A) and torch.equal(o.joints, ref.joints) and torch.equal(o.tverts, ref.tverts) and torch.equal(o.pverts, ref.pverts)
    assert maxdiff(o.R, ref.R) < 1e-7 and maxdiff(o.wverts, ref.wverts) < 1e-6 and maxdiff(o.pnorm, ref.pnorm) == 0.0
    # float64: the same operation, closer than the goldens' own tolerances
    o64 = R.pose_frame(c, F64)
    assert o64.pverts.dtype == F64 and maxdiff(o64.pverts, o.pverts) < 2e-6 and maxdiff(o64.A, o.A) < 1e-6 and maxdiff(o64.pnorm, o.pnorm) < 5e-4      # thin triangles: the float32 sum of cross products


@pytest.mark.parametrize('name', list(R.BODY_CASES))
def test_body_cases_are_well_conditioned(name):
    """the blended big-pose 3 x 3 is inverted through adjugate / (det + 1e-8): |det| >= 0.1 keeps that epsilon (and the inverse's
    conditioning) out of the comparison.  Also what each case is there for."""
    c = R.body_case(name)
    J, tree, pose, rh, N, wk, big, mesh, padding = R.BODY_CASES[name]
    o = R.pose_frame(c, F64, padding)
    det = o.bigdet.abs()
    print(f'{name}: |det| of the blended big-pose 3 x 3: min {float(det.min()):.3f} max {float(det.max()):.3f}; depth {R.tree_depth(c.parents)}')
    assert float(det.min()) >= 0.1
    assert c.poses.shape == (J, 3) and c.tverts.shape == (N, 3) and c.weights.shape == (N, J) and bool((c.parents[1:] < np.arange(1, J)).all())
    assert np.abs(c.weights.sum(1) - 1).max() < 1e-5
    assert all(bool(torch.isfinite(o[k]).all()) for k in ('A', 'tverts', 'pverts', 'wverts', 'pnorm'))
    val = np.bincount(c.faces.reshape(-1), minlength=N)
    if mesh == 'isolated':
        assert int((val == 0).sum()) == 5 and float(o.pnorm[T(val == 0)].abs().max()) == 0.0
    if mesh == 'fan':
        assert val.max() >= 200 and (3 * len(c.faces)) % 2 == 1
    if mesh == 'degenerate':
        assert (3 * len(c.faces)) % 2 == 1 and c.faces[-1, 0] == c.faces[-1, 1]
    if mesh in ('hull', 'degenerate') and N >= 4:
        assert val.min() >= 3                                                  # closed: every vertex is on the hull
    if pose == 'near_pi':
        assert 3.14 < np.linalg.norm(c.poses, axis=1).min() and np.linalg.norm(c.poses, axis=1).max() < np.pi
    if pose == 'over_2pi':
        assert np.linalg.norm(c.poses, axis=1).min() > 2 * np.pi


def test_body_cases_cover_the_issue():
    col = lambda i: {v[i] for v in R.BODY_CASES.values()}
    assert col(0) == {1, 2, 24, 52, 65, 256} and col(1) == {'chain', 'star', 'random'}
    assert col(2) == {'zero', 'tiny', 'random', 'near_pi', 'over_2pi'} and col(3) == {'zero', 'tiny', 'random'}
    assert col(4) == {3, 255, 256, 257, 1023, 1025, 6890} and col(5) == {'onehot', 'uniform', 'four'}
    assert col(6) == {'identity', 'posed'} and col(7) == {'hull', 'isolated', 'degenerate', 'fan'} and col(8) == {0.0, 0.05}
    tv, f1, f2 = R.face_pair()
    assert f1.shape == f2.shape and int((f1 != f2).sum()) == 1
    n1, n2 = O.verts_normals(T(tv), T(f1)), O.verts_normals(T(tv), T(f2))
    assert maxdiff(n1, n2) > 1e-2


# ------------------------------------------------------------------------------------------------ b. ray generation
def test_ray_reference_reproduces_the_golden(golden):
    g = golden('rays.npz')
    for tag in ('a', 'b'):
        H, W = int(g[f'{tag}_H']), int(g[f'{tag}_W'])
        rf = R.ray_frame(H, W, g[f'{tag}_K'], g[f'{tag}_R'], g[f'{tag}_T'], g['bounds'], F32)
        m = rf.mask
        assert np.array_equal(m.reshape(H, W).numpy(), g[f'{tag}_mask'])
        assert maxdiff(rf.ray_d[m], g[f'{tag}_ray_d']) < 2e-7 and maxdiff(rf.ray_o[m], g[f'{tag}_ray_o']) < 1e-7
        assert maxdiff(rf.near[m], g[f'{tag}_near']) < 2e-6 and maxdiff(rf.far[m], g[f'{tag}_far']) < 2e-6
        # the numpy restatement the batches are built with
        ro, rd, near, far, mask = synthetic.rays_within_bounds(H, W, g[f'{tag}_K'].astype(np.float64), g[f'{tag}_R'].astype(np.float64),
                                                                g[f'{tag}_T'].astype(np.float64).reshape(3, 1), g['bounds'])
        assert np.array_equal(mask.reshape(-1), m.numpy()) and maxdiff(rf.ray_d[m], rd) < 1e-7 and maxdiff(rf.near[m], near) < 1e-6


@pytest.mark.parametrize('case', R.RAY_CASES, ids=lambda c: f'{c[0]}x{c[1]}-{c[2]}-{c[3]}')
def test_ray_cases_have_few_undecided_pixels(case):
    H, W, cam, box = case
    K, Rc, Tc, bounds = R.ray_case(*case)
    r64, r32 = R.ray_frame(H, W, K, Rc, Tc, bounds, F64), R.ray_frame(H, W, K, Rc, Tc, bounds, F32)
    dec = R.decided(r64, bounds)
    und = int((~dec).sum())
    print(f'{case}: {int(r64.mask.sum())} of {H * W} pixels in the box, {und} undecided, float32 mask flips {int((r64.mask != r32.mask).sum())}')
    assert und <= 0.01 * H * W
    assert torch.equal(r64.mask[dec], r32.mask[dec])                           # what "decided" promises
    n = int(r64.mask.sum())
    if box == 'inside':
        assert n == H * W and bool((r64.near < 0).all())
    if box == 'covering':
        assert n == H * W and bool((r64.near > 0).all())
    if box == 'one_pixel':
        assert 1 <= n <= 2
    if box == 'behind':
        assert n >= 1 and bool((r64.far[r64.mask] < 0).all())
    if box == 'off':
        assert n == 0
    if cam == 'axis':                                                          # one column and one row with a direction component of exactly 0
        d = r64.ray_d.reshape(H, W, 3)
        # (0 up to the rounding of LAPACK's inverse of K, 1e-17: inside (-1e-10, 1e-5), so the pixel takes the replacement branch)
        assert bool((d[:, W // 2, 0].abs() < 1e-10).all()) and bool((d[H // 2, :, 1].abs() < 1e-10).all())


def test_ray_cases_cover_the_issue():
    assert {(c[0], c[1]) for c in R.RAY_CASES} == {(1, 1), (1, 37), (37, 53), (48, 80), (80, 48)}
    assert {c[3] for c in R.RAY_CASES} >= {'inside', 'covering', 'one_pixel', 'behind'} and {c[2] for c in R.RAY_CASES} == {'tilted', 'axis'}
    K, Rc, Tc = R.make_camera(37, 53, 'tilted')
    assert K[0, 0] != K[1, 1] and abs(K[0, 2] - 53 / 2) > 1 and abs(Rc[0, 1]) > 0.1 and abs(np.linalg.det(Rc) - 1) < 1e-12


# ------------------------------------------------------------------------------------------------ c. AABB clip
def test_aabb_reference(golden):
    ops = {k: T(v) for k, v in golden('ops.npz').items()}
    n, f = O.get_near_far_aabb(ops['aabb_bounds'], ops['aabb_o'], ops['aabb_d'])
    assert bool(((n - ops['aabb_near']).abs() <= 1e-6 * ops['aabb_near'].abs()).all()) and bool(((f - ops['aabb_far']).abs() <= 1e-6 * ops['aabb_far'].abs()).all())
    for cnt in (1, 255, 257):
        o, d = R.aabb_case(cnt)
        n32, f32 = R.aabb(o, d, F32)
        n64, f64 = R.aabb(o, d, F64)
        assert n32.dtype == F32 and n64.dtype == F64 and bool(torch.isfinite(n64).all()) and bool(torch.isfinite(f64).all())
        rel = lambda a, b: float(((a.double() - b) .abs() / b.abs().clamp(min=1)).max())
        assert rel(n32, n64) < 1e-6 and rel(f32, f64) < 1e-6
    o, d = R.aabb_case(257)
    for v in R.AABB_SPECIAL:                                                   # every special component is there, in every axis
        assert all(bool((d[:, ax] == np.float32(v)).any()) for ax in range(3)), v
    lo, hi = T(R.AABB_BOX)
    inside = ((o > lo) & (o < hi)).all(1)
    assert bool(inside.any()) and bool(((o < lo) | (o > hi)).any(1).any()) and bool((o[:, 0] == lo[0]).any()) and bool((o[:, 2] == hi[2]).any())
    # the quirk's interval: (-1e-16, 1e-8) becomes +1e-8, its ends stay
    one = torch.zeros(1, 3)
    for v, replaced in ((0.0, True), (1e-9, True), (-1e-17, True), (1e-8, False), (-1e-16, False), (-1e-9, False)):
        n_, f_ = R.aabb(one, torch.tensor([[v, 0.6, 0.8]], dtype=F32), F32)
        comp = (1e-8 if replaced else float(np.float32(v)), float(np.float32(0.6)), float(np.float32(0.8)))
        ts = [sorted([float(lo[a]) / q, float(hi[a]) / q]) for a, q in enumerate(comp)]
        assert float(n_) == pytest.approx(max(t[0] for t in ts), rel=1e-5) and float(f_) == pytest.approx(min(t[1] for t in ts), rel=1e-5), v


# ------------------------------------------------------------------------------------------------ d. BRDF
def test_brdf_reference_reproduces_the_golden(golden):
    ops = {k: T(v) for k, v in golden('ops.npz').items()}
    c = O.odict(p2l=ops['mf_p2l'], p2c=ops['mf_p2c'], normal=ops['mf_n'], albedo=ops['mf_albedo'], rough=ops['mf_rough'].reshape(-1))
    b = R.brdf(c, F32)
    assert bool(((b - ops['mf_brdf']).abs() <= 1e-6 + 1e-4 * ops['mf_brdf'].abs()).all())
    b64 = R.brdf(c, F64)
    assert b64.dtype == F64 and bool(((b64 - ops['mf_brdf']).abs() <= 1e-6 + 1e-4 * ops['mf_brdf'].abs()).all())


@pytest.mark.parametrize('size', R.BRDF_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_brdf_cases_have_few_pairs_near_a_switch(size):
    L, N = size
    c = R.brdf_case(L, N)
    near = R.brdf_near_switch(c)
    print(f'{L} x {N}: {int(near.sum())} of {L * N} pairs near a switch')
    assert int(near.sum()) <= 0.02 * L * N
    for kw in ({}, {'lambert_only': True}, {'glossy_only': True}):
        b32, b64 = R.brdf(c, F32, **kw), R.brdf(c, F64, **kw)
        assert b32.shape == (L, N, 3) and bool(torch.isfinite(b64).all()) and bool(torch.isfinite(b32).all())
        keep = ~near
        scale = max(float(b64[keep].abs().max()), 1e-30)
        e = float((b32.double() - b64)[keep].abs().max()) / scale
        print(f'    {kw}: float32 reference vs float64 on the kept pairs: max {e:.2e} of max |ref| {scale:.3e}')
        assert e < 1e-3                                                         # away from the switches float32 follows float64
    if (L, N) != (1, 1):
        v, n = torch.nn.functional.normalize(c.p2c.double(), dim=-1), c.normal.double()
        vn = (v * n).sum(-1)
        for target in R.V_DOT_N:
            assert bool(((vn - target).abs() < 1e-7).any()), target
        assert bool((vn == 0).any())                                           # v.n = 0 is exact
        assert {float(np.float32(x)) for x in R.ROUGH} == set(c.rough.tolist())
        assert bool((c.albedo == 0).all(1).any()) and bool((c.albedo == 1).all(1).any())
        l = torch.nn.functional.normalize(c.p2l.double(), dim=-1)
        assert float((l[0, 0] - v[0]).abs().max()) < 1e-7 and float((l[1, 0] + v[0]).abs().max()) < 1e-7       # l = v, l = -v
        assert near[1, 0]                                                      # ... whose half vector is 0: left out, the kernel must stay finite
    if L > 2:
        assert bool(((c.p2l[2] * c.normal).sum(-1) == 0).any())                # l perpendicular to n
    if (L, N) == (3, 85):
        assert bool((c.normal[84] == 0).all()) and bool(near[:, 84].all())


# ------------------------------------------------------------------------------------------------ e. envmap
def test_envmap_references_reproduce_the_golden(golden):
    g = golden('envmap.npz')
    lights = synthetic.make_novel_lights(3, 0)
    repeat = int(g['repeat'])
    for index in (0, 5, 37, 128 + 77, 2 * 128 + 127):
        i, j = index // (32 * repeat), index % (32 * repeat)
        probe = lights[list(lights.keys())[i]].probe[0]
        assert maxdiff(R.shift_envmap(probe, 32 / (32 * repeat) * j), g[f'rot{index}_probe']) < 1e-6
        img = T(g['images'][i])
        s = img.shape[1] / (32 * repeat) * j
        assert maxdiff(R.shift_envmap(img, s), g[f'rot{index}_image']) < 1e-6
        assert torch.equal(R.shift_envmap(img, s), O.shift_envmap(img, s))     # float32: the oracle's, bit for bit
        assert maxdiff(R.shift_envmap(img.double(), s), g[f'rot{index}_image']) < 1e-6
    H, W = int(g['H']), int(g['W'])
    uW = int(W * 0.2)
    uH = int(uW * 16 / 32)
    out = R.add_light_probe(T(g['rgb_in']), lights['probe00'].probe[0], H, W, T(g['cam_R']), uH, uW)
    assert maxdiff(out, g['rgb_out']) < 1e-5
    out64 = R.add_light_probe(T(g['rgb_in']).double(), lights['probe00'].probe[0], H, W, T(g['cam_R']), uH, uW)
    assert out64.dtype == F64 and maxdiff(out64, g['rgb_out']) < 1e-5


def test_envmap_cases():
    for (H, W, C) in R.ENV_SHAPES:
        img = R.env_image(H, W, C)
        for s in R.ENV_SHIFTS(W):
            a, b = R.shift_envmap(img, s), R.shift_envmap(img.double(), s)
            assert a.shape == (H, W, C) and maxdiff(a, b) < 1e-5
            assert torch.equal(a, O.shift_envmap(img, s))
        for s in (0.0, float(W), float(-W)):                                   # whole turns: the image itself
            assert maxdiff(R.shift_envmap(img.double(), s), img) < 1e-12
    Hh, Ww = R.PROBE_IMAGE
    rgb = R.env_image(Hh, Ww, 3, seed=1).reshape(-1, 3)
    for cam in R.probe_cams():
        for (ph, pw) in R.PROBE_SIZES:
            probe = R.env_image(ph, pw, 3, seed=2)
            for (uH, uW) in R.PROBE_INSETS:
                a, b = R.add_light_probe(rgb, probe, Hh, Ww, cam, uH, uW), R.add_light_probe(rgb.double(), probe, Hh, Ww, cam, uH, uW)
                assert maxdiff(a, b) < 1e-4
                inset = torch.zeros(Hh, Ww, dtype=torch.bool)
                inset[:uH, :uW] = True
                assert torch.equal(a.reshape(Hh, Ww, 3)[~inset], rgb.reshape(Hh, Ww, 3)[~inset])
                if (ph, pw) == (1, 1) and uH:
                    assert maxdiff(a.reshape(Hh, Ww, 3)[inset], probe[0, 0].expand(int(inset.sum()), 3)) < 1e-6


# ------------------------------------------------------------------------------------------------ f. visualiser
def test_image_reference_reproduces_the_golden(golden):
    from test_oracle_golden import _visual_inputs
    g = golden('visual.npz')
    out, batch, cfg = _visual_inputs(golden)
    H = W = int(batch.meta.H[0])
    maps = O.odict({k: v[0] for k, v in out.items() if k.endswith('_map')})
    pix = batch.mask_at_box[0].reshape(-1).nonzero()[:, 0]
    uW = int(W * cfg.probe_size_ratio)
    uH = int(uW * cfg.env_h / cfg.env_w)
    for kind in R.KINDS:
        for dt in (F32, F64):
            img = R.generate_image(maps, kind, cfg, H, W, pix, cam_R=batch.cam_R[0], tbounds=batch.tbounds[0], dtype=dt)
            rgb = R.add_light_probe(img[..., :3].reshape(-1, 3), out['envmap']['probe'][0], H, W, batch.cam_R[0].to(dt), uH, uW).reshape(H, W, 3)
            img = torch.cat([rgb, img[..., 3:]], -1)
            r = T(g[f'img_{kind}'])
            assert img.dtype == dt and bool((img.isnan() == r.isnan()).all()), kind
            assert float((img - r).nan_to_num(0.0).abs().max()) < 2e-5, (kind, dt)
    # the clamp only acts where the reference raises: more hits than k here, so the unclamped rank gives the same image
    a, b = (R.generate_image(maps, 'Depth', cfg, H, W, pix, dtype=F32, clamp=c) for c in (True, False))
    assert torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))


def test_image_cases():
    cfg = make_cfg('relight')
    assert {'normalize_shading', 'normalize_specular', 'tonemapping_albedo', 'min_clip', 'bg_brightness'} <= set(cfg.keys())
    for P in R.IMAGE_P:
        maps, H, W, pix, tb = R.image_case(P)
        assert H != W and H * W > P and bool((pix[1:] > pix[:-1]).all())
        for name, (d, a) in R.depth_variants(maps).items():
            m = O.odict(maps)
            m.depth_map, m.acc_map = d, a
            i32, i64 = (R.generate_image(m, 'Depth', cfg, H, W, pix, dtype=dt) for dt in (F32, F64))
            assert bool((i32.isnan() == i64.isnan()).all()), (P, name)
            k, hits = int(0.01 * P), int((a != 0).sum())
            if name == 'one_hit' and k > hits:                                 # the reference raises here; the clamped rank does not
                with pytest.raises(RuntimeError):
                    R.generate_image(m, 'Depth', cfg, H, W, pix, clamp=False)
            if name == 'no_hit':                                               # stretched between 0 and 1
                assert torch.equal(i32.reshape(-1, 4)[pix][:, 0], d.clip(0, 1))
            if name in ('nans', 'one_negative_nan', 'all_equal_low') or (name == 'minus_inf' and k == 1):     # topk's max / min carry a NaN; inf / inf; 0 / 0
                assert bool(i32.reshape(-1, 4)[pix][:, :3].isnan().all()), (P, name)
            if name == 'all_equal_high':
                assert bool((i32.reshape(-1, 4)[pix][:, :3] == 1).all())
            if name == 'plus_inf' and k == 1:
                assert int(i32.isnan().sum()) == 3
    with pytest.raises(ValueError):
        m, H, W, pix, tb = R.image_case(99)
        R.generate_image(m, 'Depth', cfg, H, W, pix)


# ------------------------------------------------------------------------------------------------ g, h
def test_blend_reference_is_blend_output():
    r = np.random.default_rng(5)
    F_, P = 300, 120
    inds = T(r.permutation(F_)[:P])
    acc = T(r.uniform(0, 1, F_).astype(np.float32))
    for C_ in (1, 3):
        grd, hum = T(r.uniform(0, 1, (F_, C_)).astype(np.float32)), T(r.uniform(0, 1, (P, C_)).astype(np.float32))
        ret = O.blend_output_(acc, inds, O.odict(rgb_map=grd), O.odict(rgb_map=hum, acc_map=torch.zeros(P)))
        assert torch.equal(R.blend_ground(grd, hum, inds, acc, F_, C_), ret.rgb_map)
        only = O.blend_output_(acc, inds, O.odict(rgb_map=grd), O.odict(acc_map=torch.zeros(P)))
        assert torch.equal(R.blend_ground(grd, None, inds, acc, F_, C_), only.rgb_map)

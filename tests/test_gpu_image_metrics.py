"""ra_image_metrics (csrc/ra_metrics.hip) through Engine.image_metrics, and the Evaluator on top of it.  Run with `-m gpu` on an MI355X.

Parity rule — section 12's, one precision up, no new constant: per output, the kernel's distance from the truth (image_metrics_ref.truth,
longdouble) is at most the larger of 10 x the float64 restatement's own distance (scikit-image's algorithm on scipy) and 8 double unit
roundoffs of the value.  The float32 restatement's distance — scikit-image's own arithmetic on the reference's float32 images — is printed
beside; the kernel must be far below it.  Bit-identity claims compare the raw 64-bit patterns.

Every test prints its figures before it asserts (pytest -s); DESIGN.md section 14 holds the record.
"""
import numpy as np
import pytest
import torch

import image_metrics_ref as R
from relightableavatar_amd import _lib, synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.evaluators import Evaluator, make_evaluator
from test_oracle_image_metrics import case

pytestmark = pytest.mark.gpu

KEYS = ('mse', 'psnr', 'ssim')
_state = []


def build(mode, **kw):
    from relightableavatar_amd.networks import make_network
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    dev = torch.device('cuda:0')
    cfg = make_cfg(mode, **kw)
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=mode in ('relight', 'novel_light'), cfg=cfg))
    return cfg, net.to(dev).eval(), dev


def engine():
    if not _state:
        cfg, net, dev = build('novel_light')
        _state.append((cfg, net, net.engine(), dev))
    return _state[0]


def metrics(pred, gt, H, W, **kw):
    """numpy float64 (4,) of one call; pred / gt: numpy (..., 3) float32"""
    eng, dev = engine()[2], engine()[3]
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)      # a copy: the shared cases are read-only
    for k in ('pix', 'mask'):
        if k in kw:
            kw[k] = t(kw[k])
    out = eng.image_metrics(t(pred.reshape(-1, 3)), t(gt.reshape(-1, 3)), H, W, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_rule(tag, got, t, b, c=None):
    for i, k in enumerate(KEYS):
        e, tol = R.dist(got[i], t[k]), R.allowed(b[k], t[k])
        beside = '' if c is None else f', float32 restatement {float(R.dist(c[k], t[k])):.2e}'
        print(f'{tag} {k}: truth {float(t[k]):.17g}, kernel off by {float(e):.2e}, float64 restatement {float(R.dist(b[k], t[k])):.2e}{beside}, allowed {float(tol):.2e}')
    for i, k in enumerate(KEYS):
        assert R.dist(got[i], t[k]) <= R.allowed(b[k], t[k]), (tag, k, got[i], t[k])
    assert got[3] == t['windows'], (tag, got[3], t['windows'])


# ---------------------------------------------------------------------------------------------- 1. symbols
def test_native_symbols_are_loaded():
    eng = engine()[2]
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert eng.lib.ra_abi_version() == 9 and hasattr(eng.lib, 'ra_image_metrics')


# ---------------------------------------------------------------------------------------------- 2. parity on full images
@pytest.mark.parametrize('name', R.SETS)
def test_parity_full_images(name):
    for H, W in R.SIZES:          # 7x7: one window; 37 / 38 / 39: around the 32-window tile; 256x300: 80 tiles, 38 pixel-pass workgroups
        pred, gt, t, b, c = case(name, H, W)
        check_rule(f'{name} {H}x{W}', metrics(pred, gt, H, W), t, b, c)


# ---------------------------------------------------------------------------------------------- 3. ray lists
def sparse_rays(H=64, W=64):
    pred, gt = case('sparse', H, W)[:2]
    y0, x0, h, w = R.box_of(H, W)
    mask = np.zeros((H, W), bool)
    mask[y0:y0 + h, x0:x0 + w] = True
    pix = np.flatnonzero(mask.reshape(-1))
    return pred, gt, mask, pix, pred.reshape(-1, 3)[pix], gt.reshape(-1, 3)[pix]


@pytest.mark.parametrize('bg', [0.0, 1.0])
def test_ray_list_equals_assembled_image(bg):
    H = W = 64
    pred, gt, mask, pix, rp, rg = sparse_rays(H, W)
    assert 0 < pix.size < H * W
    ip, ig = R.assemble(rp, pix, H, W, bg), R.assemble(rg, pix, H, W, bg)
    full = metrics(ip, ig, H, W)
    rays = metrics(rp, rg, H, W, pix=pix, bg=bg)
    perm = np.random.default_rng(1).permutation(pix.size)
    shuffled = metrics(rp[perm], rg[perm], H, W, pix=pix[perm], bg=bg)
    print(f'bg {bg}: full image {full}, ray list {rays}, permuted {shuffled}')
    assert np.array_equal(bits(full), bits(rays)) and np.array_equal(bits(full), bits(shuffled))
    check_rule(f'assembled bg {bg}', rays, R.truth(ip, ig), R.restated(ip, ig))


# ---------------------------------------------------------------------------------------------- 4. crop to the mask's rectangle
def test_crop_to_mask():
    H = W = 64
    pred, gt, mask, pix, rp, rg = sparse_rays(H, W)
    x, y, w, h = R.bounding_rect(mask)
    cp, cg = pred[y:y + h, x:x + w], gt[y:y + h, x:x + w]
    whole = metrics(pred, gt, H, W)
    cropped = metrics(pred, gt, H, W, mask=mask.astype(np.uint8))
    direct = metrics(cp, cg, h, w)
    from_rays = metrics(rp, rg, H, W, pix=pix, mask=mask.astype(np.uint8))
    print(f'crop_to_mask {cropped}, the cropped arrays {direct}, ray list + mask {from_rays}, whole image {whole}')
    assert np.array_equal(bits(cropped[2:]), bits(direct[2:])) and np.array_equal(bits(from_rays[2:]), bits(direct[2:]))
    assert np.array_equal(bits(cropped[:2]), bits(whole[:2]))               # the crop concerns the SSIM alone
    assert cropped[3] == (h - 6) * (w - 6) != whole[3]
    t, b = R.truth(cp, cg), R.restated(cp, cg)
    for k, i in (('ssim', 2),):
        print(f'cropped ssim: kernel off by {float(R.dist(cropped[i], t[k])):.2e}, allowed {float(R.allowed(b[k], t[k])):.2e}')
        assert R.dist(cropped[i], t[k]) <= R.allowed(b[k], t[k])
    # a single mask pixel far away widens the rectangle
    m2 = mask.copy()
    m2[3, 60] = True
    x2, y2, w2, h2 = R.bounding_rect(m2)
    wide = metrics(pred, gt, H, W, mask=m2.astype(np.uint8))
    assert np.array_equal(bits(wide[2:]), bits(metrics(pred[y2:y2 + h2, x2:x2 + w2], gt[y2:y2 + h2, x2:x2 + w2], h2, w2)[2:]))


def test_rectangles_without_a_window():
    H = W = 64
    pred, gt = case('noise', H, W)[:2]
    want = metrics(pred, gt, H, W)
    low = np.zeros((H, W), np.uint8)
    low[20:25, 10:50] = 1                                                   # 5 rows x 40 columns
    for tag, m in (('5x40 rectangle', low), ('empty mask', np.zeros((H, W), np.uint8))):
        got = metrics(pred, gt, H, W, mask=m)
        print(f'{tag}: {got}')
        assert np.isnan(got[2]) and got[3] == 0 and np.array_equal(bits(got[:2]), bits(want[:2]))
    p5, g5 = case('noise', 64, 64)[0][:5, :40], case('noise', 64, 64)[1][:5, :40]      # an image lower than the window
    got = metrics(p5, g5, 5, 40)
    t = R.truth(p5, g5)
    assert np.isnan(got[2]) and got[3] == 0 and R.dist(got[0], t['mse']) <= 8 * R.U * t['mse']


# ---------------------------------------------------------------------------------------------- 5. MSE modes
def test_mse_modes():
    H = W = 64
    pred, gt, mask, pix, rp, rg = sparse_rays(H, W)
    P = pix.size
    over_rays = metrics(rp, rg, H, W, pix=pix, mse_over_rays=True)
    whole = metrics(rp, rg, H, W, pix=pix)
    t_mse, t_psnr = R.mse_psnr(rp, rg)
    b_mse, b_psnr = R.mse_psnr(rp, rg, np.float64)
    print(f'over the {P} rays: mse {over_rays[0]:.17g} (truth {float(t_mse):.17g}), psnr {over_rays[1]:.17g} (truth {float(t_psnr):.17g}); whole image mse {whole[0]:.17g}')
    assert R.dist(over_rays[0], t_mse) <= R.allowed(b_mse, t_mse) and R.dist(over_rays[1], t_psnr) <= R.allowed(b_psnr, t_psnr)
    scaled = t_mse * P / (H * W)
    assert R.dist(whole[0], scaled) <= R.allowed(np.float64(b_mse) * P / (H * W), scaled)
    assert np.array_equal(bits(over_rays[2:]), bits(whole[2:]))             # the SSIM does not depend on the mode


# ---------------------------------------------------------------------------------------------- 6. exact cases
def test_exact_cases():
    eng, dev = engine()[2], engine()[3]
    for name in R.SETS:
        x = case(name, 33, 70)[0]
        got = metrics(x, x, 33, 70)
        print(f'{name} against itself: {got}')
        assert got[0] == 0.0 and np.isposinf(got[1]) and got[2] == 1.0 and got[3] == 27 * 64
    pred, gt = case('noise', 256, 300)[:2]
    a, b = metrics(pred, gt, 256, 300), metrics(pred, gt, 256, 300)
    assert np.array_equal(bits(a), bits(b))
    sentinel = torch.full((3, 4), -12345.678, dtype=torch.float64, device=dev)
    table = sentinel.clone()
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    r = eng.image_metrics(tp, tg, 256, 300, out=table[1])
    torch.cuda.synchronize()
    assert r.data_ptr() == table[1].data_ptr()
    assert torch.equal(table[0], sentinel[0]) and torch.equal(table[2], sentinel[2]) and np.array_equal(bits(table[1].cpu().numpy()), bits(a))


def test_argument_errors():
    eng, dev = engine()[2], engine()[3]
    x = torch.zeros(10, 3, device=dev)
    with pytest.raises(_lib.RaError, match='pixel indices'):
        eng.image_metrics(x, x, 8, 8)
    with pytest.raises(_lib.RaError, match='bad sizes'):
        eng.image_metrics(torch.zeros(80, 3, device=dev), torch.zeros(80, 3, device=dev), 8, 8, pix=torch.zeros(80, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        eng.image_metrics(x, x, 8, 8, pix=torch.zeros(9, dtype=torch.int64, device=dev))
    # a pixel index outside the image drops its ray (include/relightableavatar.h)
    pix = torch.tensor([0, 1, -5, 64, 1 << 40, 7, 8, 9, 10, 11], dtype=torch.int64, device=dev)
    got = eng.image_metrics(torch.ones(10, 3, device=dev), x, 8, 8, pix=pix, mse_over_rays=True)
    torch.cuda.synchronize()
    assert got[0].item() == 0.7


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_evaluator_end_to_end(golden):
    """The relit synthetic frame of tests/test_gpu_heads.py, built the same way (a 128 x 128 frame whose 12 x 12 window of rays is the ray
    list).  No synchronisation inside evaluate: asserted with torch's sync debug mode 'error', under which any synchronising torch call
    (an .item() of a device tensor, a nonzero(), a blocking copy) raises; the library's part is asynchronous by construction
    (ra_image_metrics only enqueues launches; its scratch is allocated on the first call of a size, which the warm-up call makes)."""
    from relightableavatar_amd.renderer import make_renderer
    ref = golden('frame_novel.npz')
    cfg, net, eng, dev = engine()
    H = int(ref['H'])
    batch = synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, crop=int(ref['crop']), n_novel_lights=3), dev)
    maps = make_renderer(cfg, net).render(batch)['probe00']
    rgb = maps.rgb_map.reshape(1, -1, 3)
    P = rgb.shape[1]
    assert P == int(ref['crop']) ** 2 < H * H
    g = torch.Generator().manual_seed(0)
    targets = [(rgb.cpu() + 0.02 * (k + 1) * torch.randn(rgb.shape, generator=g)).clamp(0, 1).to(dev) for k in range(2)]
    ev = make_evaluator(cfg)
    Evaluator.engine = eng
    try:
        eng.image_metrics(rgb[0], targets[0][0], H, H, pix=torch.arange(P, device=dev))      # warm-up: the scratch of this size
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            for tgt in targets:
                batch.rgb = tgt
                ev.evaluate(synthetic.dotdict(rgb_map=rgb), batch)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert len(ev) == 2
        mean = ev.summarize()
    finally:
        Evaluator.engine = None
    pix = np.flatnonzero(batch.mask_at_box[0].cpu().numpy())
    want = {k: [] for k in KEYS}
    floor = {k: [] for k in KEYS}
    for tgt in targets:
        ip = R.assemble(rgb[0].cpu().numpy(), pix, H, H, float(cfg.bg_brightness))
        ig = R.assemble(tgt[0].cpu().numpy(), pix, H, H, float(cfg.bg_brightness))
        t, b = R.truth(ip, ig), R.restated(ip, ig)
        for k in KEYS:
            want[k].append(t[k])
            floor[k].append(R.allowed(b[k], t[k]))
    assert sorted(mean) == sorted(KEYS) and len(ev) == 0 and [len(ev.metrics[k]) for k in KEYS] == [2, 2, 2]
    for k in KEYS:
        t, tol = np.mean(want[k], dtype=np.longdouble), max(floor[k]) + 2 * R.U * abs(np.mean(want[k], dtype=np.longdouble))   # + the mean's own rounding
        print(f'evaluator {k}: mean {mean[k]:.17g}, truth {float(t):.17g}, off by {float(R.dist(mean[k], t)):.2e}, allowed {float(tol):.2e}')
        assert R.dist(mean[k], t) <= tol
    with pytest.raises(RuntimeError, match='no frame'):
        ev.summarize()

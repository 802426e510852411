"""ra_lpips (csrc/ra_lpips.hip) through Engine.lpips / Engine.lpips_features, and the Evaluator's fourth key.  Run with `-m gpu` on an MI355X.

Parity rule — the project's 10 x float32 rule, no new constant (lpips_ref.py holds the three restatements; weights are seeded and synthetic):
  per tap   the kernel's max |error| against the float64 truth (a) over the whole activation tensor is at most 10 x the float32
            restatement (b)'s own max |error| against (a), measured in the same test;
  outputs   each of the six outputs is within max(10 x (b)'s distance from (a), 8 x 2^-24 of the value) of (a).
Bit-identity claims compare the raw 64-bit patterns.  Every test prints its figures before it asserts (pytest -s); DESIGN.md section 16
holds the record.
"""
import numpy as np
import pytest
import torch

import image_metrics_ref as IM
import lpips_ref as R
from relightableavatar_amd import _lib, synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.evaluators import make_evaluator

pytestmark = pytest.mark.gpu

_state = []


def engine(seed=None):
    """cfg, net, engine, device — one network for the module.  seed: load that weight set (a second call replaces the first); None: keep
    the set the engine holds, seed 0 on the first call"""
    from relightableavatar_amd.networks import make_network
    if not _state:
        if not torch.cuda.is_available():
            pytest.skip('no GPU')
        dev = torch.device('cuda:0')
        cfg = make_cfg('novel_light')
        net = make_network(cfg)
        net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
        net = net.to(dev).eval()
        _state.append([cfg, net, net.engine(), dev, None])
    st = _state[0]
    if seed is None:
        seed = 0 if st[4] is None else st[4]
    if st[4] != seed:
        st[2].lpips_load(R.weights(seed))
        st[4] = seed
    return st[0], st[1], st[2], st[3]


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(dev)      # a copy: the shared cases are read-only


def lpips(x0, x1, H, W, **kw):
    """numpy float64 (6,) of one call; x0 / x1: numpy (..., 3) float32"""
    _, _, eng, dev = engine()
    for k in ('pix', 'mask'):
        if k in kw:
            kw[k] = to_dev(kw[k], dev)
    out = eng.lpips(to_dev(x0.reshape(-1, 3), dev), to_dev(x1.reshape(-1, 3), dev), H, W, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_outputs(tag, got, t, b):
    for i in range(6):
        print(f'{tag} out[{i}]: truth {t[i]:.17g}, kernel off by {float(IM.dist(got[i], t[i])):.2e}, float32 restatement '
              f'{float(IM.dist(b[i], t[i])):.2e}, allowed {float(R.allowed(b[i], t[i])):.2e}')
    for i in range(6):
        assert IM.dist(got[i], t[i]) <= R.allowed(b[i], t[i]), (tag, i, got[i], t[i])


def check_taps(tag, img, t0, b0):
    _, _, eng, dev = engine()
    sizes = R.tap_sizes(*img.shape[:2])
    worst = []
    for k in range(5):
        f = eng.lpips_features(to_dev(img, dev), k)
        torch.cuda.synchronize()
        assert tuple(f.shape) == (t0[k].shape[0],) + sizes[k] == tuple(t0[k].shape)
        e = float((f.cpu().double() - t0[k]).abs().max())
        e32 = float((b0[k].double() - t0[k]).abs().max())
        print(f'{tag} tap {k} {tuple(f.shape)}: max |activation| {float(t0[k].max()):.3g}, kernel max |error| {e:.2e}, float32 restatement {e32:.2e} '
              f'(ratio {e / e32 if e32 else float("inf"):.2f})')
        worst.append((e, e32))
    for k, (e, e32) in enumerate(worst):
        assert e <= 10 * e32, (tag, k, e, e32)


def edge_sizes():
    """for conv1 and conv2: the image size whose M (output pixels of both images) is the largest below the kernel's M tile, the one that fills
    it exactly where one exists, and the smallest above it — found from the kernel's own constant"""
    bm = _lib.lib().ra_lpips_tile_m()
    out = []
    for tap in (0, 1):
        below, exact, above = None, None, None
        for H in range(31, 160):
            for W in range(H, 160):
                h, w = R.tap_sizes(H, W)[tap]
                m = 2 * h * w
                if m < bm and (below is None or m > below[0]):
                    below = (m, H, W)
                if m == bm and exact is None:
                    exact = (m, H, W)
                if m > bm and (above is None or m < above[0]):
                    above = (m, H, W)
        out += [s for s in (below, exact, above) if s is not None]
    return bm, out


# ---------------------------------------------------------------------------------------------- 1. symbols, errors
def test_native_symbols_and_load_order():
    """before any load the call is refused (a context of its own, so the order of the tests does not matter)"""
    from relightableavatar_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    dev = torch.device('cuda:0')
    bare = Engine(make_cfg('novel_light'), dev, relight=True)                          # a context of its own: no weights of any kind
    assert 'librelightableavatar_hip.so' in open('/proc/self/maps').read()
    assert bare.lib.ra_abi_version() == 9 and hasattr(bare.lib, 'ra_lpips') and not bare.lpips_loaded()
    x = torch.zeros(64 * 64, 3, device=dev)
    with pytest.raises(_lib.RaError, match='lpips weights not loaded'):
        bare.lpips(x, x, 64, 64)
    with pytest.raises(_lib.RaError, match='lpips weights not loaded'):
        bare.lpips_features(x.reshape(64, 64, 3), 0)
    _, _, eng, _ = engine()
    assert eng.lpips_loaded()
    with pytest.raises(_lib.RaError, match='pixel indices'):
        eng.lpips(x[:10], x[:10], 64, 64)
    with pytest.raises(_lib.RaError, match='bad sizes'):
        eng.lpips(torch.zeros(80, 3, device=dev), torch.zeros(80, 3, device=dev), 8, 8, pix=torch.zeros(80, dtype=torch.int64, device=dev))
    with pytest.raises(KeyError, match='missing conv0.weight'):
        eng.lpips_load({})


# ---------------------------------------------------------------------------------------------- 2. parity
@pytest.mark.parametrize('size', R.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', ['noise', 'inverse'])
def test_parity_outputs(name, size):
    H, W = size
    x0, x1, t, b, _, _ = R.case(name, H, W)
    check_outputs(f'{name} {H}x{W}', lpips(x0, x1, H, W), t, b)


@pytest.mark.parametrize('name', ['smooth', 'sparse'])
def test_parity_outputs_other_sets(name):
    x0, x1, t, b, _, _ = R.case(name, 64, 64)
    check_outputs(f'{name} 64x64', lpips(x0, x1, 64, 64), t, b)


@pytest.mark.parametrize('size', [(31, 31), (35, 35), (39, 39), (64, 64), (67, 130)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_parity_taps(size):
    H, W = size
    x0, _, _, _, t0, b0 = R.case('noise', H, W)
    check_taps(f'noise {H}x{W}', x0, t0, b0)


def test_parity_around_the_m_tile():
    bm, sizes = edge_sizes()
    print(f'M tile {bm}: sizes {sizes}')
    assert len(sizes) >= 4
    for m, H, W in sizes:
        x0, x1, t, b, t0, b0 = R.case('noise', H, W)
        check_taps(f'M = {m} ({H}x{W})', x0, t0, b0)
        check_outputs(f'M = {m} ({H}x{W})', lpips(x0, x1, H, W), t, b)


# ---------------------------------------------------------------------------------------------- 3. exact properties
def test_exact_properties():
    _, _, eng, dev = engine()
    for name in R.SETS:
        x = R.case(name, 64, 64)[0]
        got = lpips(x, x, 64, 64)
        print(f'{name} against itself: {got}')
        assert np.array_equal(bits(got), bits(np.zeros(6)))
    x0, x1 = R.case('noise', 67, 130)[:2]
    a, b, c = lpips(x0, x1, 67, 130), lpips(x1, x0, 67, 130), lpips(x0, x1, 67, 130)
    print(f'(a, b) {a}\n(b, a) {b}')
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)) and a[0] > 0
    sentinel = torch.full((3, 6), -12345.678, dtype=torch.float64, device=dev)
    table = sentinel.clone()
    r = eng.lpips(to_dev(x0, dev), to_dev(x1, dev), 67, 130, out=table[1])
    torch.cuda.synchronize()
    assert r.data_ptr() == table[1].data_ptr()
    assert torch.equal(table[0], sentinel[0]) and torch.equal(table[2], sentinel[2]) and np.array_equal(bits(table[1].cpu().numpy()), bits(a))


def sparse_rays(H=64, W=64):
    x0, x1 = R.case('sparse', H, W)[:2]
    y0, xl, h, w = IM.box_of(H, W)
    mask = np.zeros((H, W), bool)
    mask[y0:y0 + h, xl:xl + w] = True
    pix = np.flatnonzero(mask.reshape(-1))
    return x0, x1, mask, pix, x0.reshape(-1, 3)[pix], x1.reshape(-1, 3)[pix]


@pytest.mark.parametrize('bg', [0.0, 1.0])
def test_ray_list_equals_assembled_image(bg):
    H = W = 64
    x0, x1, mask, pix, r0, r1 = sparse_rays(H, W)
    assert 0 < pix.size < H * W
    i0, i1 = IM.assemble(r0, pix, H, W, bg), IM.assemble(r1, pix, H, W, bg)
    full = lpips(i0, i1, H, W)
    rays = lpips(r0, r1, H, W, pix=pix, bg=bg)
    perm = np.random.default_rng(1).permutation(pix.size)
    shuffled = lpips(r0[perm], r1[perm], H, W, pix=pix[perm], bg=bg)
    print(f'bg {bg}: full image {full}, ray list {rays}, permuted {shuffled}')
    assert np.array_equal(bits(full), bits(rays)) and np.array_equal(bits(full), bits(shuffled))
    sd = R.weights(0)
    check_outputs(f'assembled bg {bg}', rays, R.lpips(i0, i1, sd, torch.float64)[0], R.lpips(i0, i1, sd, torch.float32)[0])


def test_crop_to_mask():
    """bit for bit: the cropped planes are written at the origin, so every later kernel sees the rows, tiles and summation order of a call
    on the cropped arrays"""
    H, W = 96, 120
    x0, x1 = R.case('noise', H, W)[:2]
    mask = np.zeros((H, W), bool)
    mask[20:61, 30:97] = True                                                       # a 41 x 67 rectangle
    mask[25, 40] = False
    x, y, w, h = IM.bounding_rect(mask)
    assert (h, w) == (41, 67)
    c0, c1 = x0[y:y + h, x:x + w], x1[y:y + h, x:x + w]
    whole = lpips(x0, x1, H, W)
    cropped = lpips(x0, x1, H, W, mask=mask.astype(np.uint8))
    direct = lpips(c0, c1, h, w)
    pix = np.random.default_rng(2).permutation(H * W)
    from_rays = lpips(x0.reshape(-1, 3)[pix], x1.reshape(-1, 3)[pix], H, W, pix=pix, mask=mask.astype(np.uint8))
    print(f'crop_to_mask {cropped}\nthe cropped arrays {direct}\nray list + mask {from_rays}\nwhole image {whole}')
    assert np.array_equal(bits(cropped), bits(direct)) and np.array_equal(bits(from_rays), bits(direct))
    assert not np.array_equal(bits(cropped), bits(whole))
    sd = R.weights(0)
    check_outputs('cropped', cropped, R.lpips(c0, c1, sd, torch.float64)[0], R.lpips(c0, c1, sd, torch.float32)[0])


def test_below_31_gives_nans():
    H = W = 64
    x0, x1 = R.case('noise', H, W)[:2]
    low = np.zeros((H, W), np.uint8)
    low[10:40, 5:45] = 1                                                            # 30 rows x 40 columns
    for tag, got in (('30x40 rectangle', lpips(x0, x1, H, W, mask=low)), ('empty mask', lpips(x0, x1, H, W, mask=np.zeros((H, W), np.uint8))),
                     ('30x40 image', lpips(x0[:30, :40], x1[:30, :40], 30, 40)), ('40x30 image', lpips(x0[:40, :30], x1[:40, :30], 40, 30))):
        print(f'{tag}: {got}')
        assert np.isnan(got).all() and got.shape == (6,)
    ok = np.zeros((H, W), np.uint8)
    ok[10:41, 5:36] = 1                                                             # 31 x 31: the smallest rectangle with a value
    got = lpips(x0, x1, H, W, mask=ok)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(lpips(x0[10:41, 5:36], x1[10:41, 5:36], 31, 31)))


def test_second_weight_set_replaces_the_first():
    x0, x1, t0 = R.case('inverse', 64, 64)[:3]
    first = lpips(x0, x1, 64, 64)
    try:
        engine(seed=1)
        _, _, t1, b1, _, _ = R.case('inverse', 64, 64, seed=1)
        second = lpips(x0, x1, 64, 64)
        print(f'seed 0: {first[0]:.17g} (truth {t0[0]:.17g}); seed 1: {second[0]:.17g} (truth {t1[0]:.17g})')
        assert abs(t1[0] - t0[0]) > 1e-3 * t0[0]
        check_outputs('seed 1', second, t1, b1)
    finally:
        engine(seed=0)
    assert np.array_equal(bits(lpips(x0, x1, 64, 64)), bits(first))


# ---------------------------------------------------------------------------------------------- 4. end to end
def test_evaluator_end_to_end(golden):
    """The 128 x 128 relit frame of test_gpu_image_metrics.py::test_evaluator_end_to_end, built the same way, with LPIPS weights loaded.
    No synchronisation inside evaluate: torch's sync debug mode 'error' (the library's part only enqueues launches; its scratch is allocated
    on the first call of a size, which the warm-up call makes).  The other three keys are those of a context without weights, bit for bit."""
    from relightableavatar_amd.engine import Engine
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
    bare = Engine(cfg, dev, relight=True)                                              # no LPIPS weights: the three-key evaluator
    means, lists = {}, {}
    for tag, e in (('with', eng), ('without', bare)):
        ev = make_evaluator(cfg)
        e.image_metrics(rgb[0], targets[0][0], H, H, pix=torch.arange(P, device=dev))   # warm-up: the scratch of this size
        if e.lpips_loaded():
            e.lpips(rgb[0], targets[0][0], H, H, pix=torch.arange(P, device=dev))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            for tgt in targets:
                batch.rgb = tgt
                ev.evaluate(synthetic.dotdict(rgb_map=rgb), batch, engine=e)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert len(ev) == 2
        means[tag] = ev.summarize()
        lists[tag] = ev.metrics
        assert len(ev) == 0
    assert sorted(means['with']) == ['lpips', 'mse', 'psnr', 'ssim'] and sorted(means['without']) == ['mse', 'psnr', 'ssim']
    for k in ('mse', 'psnr', 'ssim'):
        assert np.array_equal(bits(lists['with'][k]), bits(lists['without'][k])) and means['with'][k] == means['without'][k]
    pix = np.flatnonzero(batch.mask_at_box[0].cpu().numpy())
    sd = R.weights(0)
    want, tol = [], []
    for tgt in targets:
        i0 = IM.assemble(rgb[0].cpu().numpy(), pix, H, H, float(cfg.bg_brightness))
        i1 = IM.assemble(tgt[0].cpu().numpy(), pix, H, H, float(cfg.bg_brightness))
        t, b = R.lpips(i0, i1, sd, torch.float64)[0][0], R.lpips(i0, i1, sd, torch.float32)[0][0]
        want.append(t)
        tol.append(R.allowed(b, t))
    t = np.mean(want)
    allowed = max(tol) + 2 * IM.U * abs(t)                                             # + the mean's own rounding
    print(f"evaluator lpips: per frame {lists['with']['lpips']}, mean {means['with']['lpips']:.17g}, truth {t:.17g}, "
          f"off by {abs(means['with']['lpips'] - t):.2e}, allowed {float(allowed):.2e}")
    assert len(lists['with']['lpips']) == 2 and abs(means['with']['lpips'] - t) <= allowed

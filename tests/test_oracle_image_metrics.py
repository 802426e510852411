"""The host side of ra_image_metrics / Evaluator: the restatements agree with each other, the formula's closed forms, the library's
symbol and the evaluator's refusals.  No GPU.

Restatement bound.  (b) evaluates uxx - ux^2 in float64: the difference of two numbers of size uxx <= 1 carries an absolute error of a
few 2^-53, against C2 = 9e-4 in the factor it enters — a relative 1e-13 per window at worst, less in the mean.  1e-12 is asserted; measured
1e-16 .. 6e-15.
"""

import numpy as np
import pytest
import torch

import image_metrics_ref as R
from relightableavatar_amd import _lib, config
from relightableavatar_amd.base_utils import dotdict
from relightableavatar_amd.evaluators import Evaluator, make_evaluator

_cache = {}


def case(name, H, W):
    """pred, gt, truth, float64 restatement, float32 restatement — computed once, shared with test_gpu_image_metrics.py"""
    key = (name, H, W)
    if key not in _cache:
        pred, gt = R.make_set(name, H, W)
        pred.setflags(write=False), gt.setflags(write=False)
        _cache[key] = (pred, gt, R.truth(pred, gt), R.restated(pred, gt, np.float64), R.restated(pred, gt, np.float32))
    return _cache[key]


@pytest.mark.parametrize('name', R.SETS)
def test_restatement_agrees_with_truth(name):
    for H, W in R.SIZES:
        pred, gt, t, b, c = case(name, H, W)
        assert b['windows'] == t['windows'] == (H - 6) * (W - 6)
        for k in ('mse', 'psnr', 'ssim'):
            e, e32 = R.dist(b[k], t[k]), R.dist(c[k], t[k])
            print(f'{name} {H}x{W} {k}: truth {float(t[k]):.17g}, float64 restatement off by {float(e):.2e}, float32 by {float(e32):.2e}')
            assert e <= 1e-12 * max(abs(t[k]), 1e-3), (name, H, W, k)


def test_constant_images_closed_form():
    c1 = 0.01 ** 2
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5)):
        x, y = np.full((9, 11, 3), a, np.float32), np.full((9, 11, 3), b, np.float32)
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        assert abs(R.truth(x, y)['ssim'] - want) <= 8 * R.U and abs(R.restated(x, y)['ssim'] - want) <= 1e-12
    for name in R.SETS:
        x = case(name, 33, 70)[0]
        t, b = R.truth(x, x), R.restated(x, x)
        assert t['ssim'] == 1.0 and b['ssim'] == 1.0 and t['mse'] == 0 and np.isposinf(t['psnr']) and np.isposinf(b['psnr'])
    assert np.isnan(R.truth(np.zeros((6, 20, 3), np.float32), np.zeros((6, 20, 3), np.float32))['ssim'])


def test_bounding_rect_and_assemble():
    m = np.zeros((10, 12), bool)
    assert R.bounding_rect(m) == (0, 0, 0, 0)
    m[2, 5] = m[7, 3] = True
    assert R.bounding_rect(m) == (3, 2, 3, 6)
    rays = np.arange(6, dtype=np.float32).reshape(2, 3)
    img = R.assemble(rays, np.array([5, 0]), 2, 3, 0.5)
    assert img.dtype == np.float32 and (img[1, 2] == rays[0]).all() and (img[0, 0] == rays[1]).all() and (img[0, 1] == 0.5).all()


def test_library_exports_image_metrics():
    L = _lib.lib()
    assert hasattr(L, 'ra_image_metrics') and 'ra_image_metrics' in _lib.SYMBOLS
    assert L.ra_abi_version() == _lib.ABI_VERSION == 9
    import ctypes as C
    assert C.sizeof(_lib.ra_metrics_params) == 24
    # the argument checks come before any device is touched
    p = _lib.ra_metrics_params(H=8, W=8, bg_brightness=0.0, data_range=1.0, mse_over_rays=0, crop_to_mask=0)
    assert L.ra_image_metrics(None, C.byref(p), None, None, None, 64, None, None, None) != 0
    assert b'null argument' in L.ra_last_error()


def _batch(H, W, P=None, **extra):
    mask = torch.zeros(1, H * W, dtype=torch.bool)
    mask[0, :H * W if P is None else P] = True
    b = dotdict(mask_at_box=mask, rgb=torch.zeros(1, H * W if P is None else P, 3), meta=dotdict(H=torch.tensor([H]), W=torch.tensor([W])))
    b.update(extra)
    return b


def test_evaluator_refusals():
    cfg = config.default_cfg()
    ev = make_evaluator(cfg)
    assert isinstance(ev, Evaluator) and len(ev) == 0 and Evaluator.engine is None
    out = dotdict(rgb_map=torch.zeros(1, 64, 3))
    with pytest.raises(NotImplementedError, match='crop_bbox'):
        ev.evaluate(out, _batch(8, 8, crop_bbox=torch.zeros(1, 2, 2)))
    with pytest.raises(ValueError, match='mask_at_box selects'):
        ev.evaluate(dotdict(rgb_map=torch.zeros(1, 20, 3)), _batch(8, 8, P=21, rgb=torch.zeros(1, 20, 3)))
    with pytest.raises(ValueError, match='mask_at_box has'):
        ev.evaluate(dotdict(rgb_map=torch.zeros(1, 20, 3)), _batch(8, 9, P=20, mask_at_box=torch.ones(1, 64, dtype=torch.bool)))
    with pytest.raises(RuntimeError, match='needs the engine'):          # every check passed: only the engine is missing, no CPU fallback
        ev.evaluate(out, _batch(8, 8))
    with pytest.raises(RuntimeError, match='no frame'):
        ev.summarize()
    cfg2 = config.default_cfg()
    cfg2.eval_whole_img = False
    ev2 = make_evaluator(cfg2)
    try:
        with pytest.raises(NotImplementedError, match='eval_whole_img'):
            ev2.evaluate(dotdict(rgb_map=torch.zeros(1, 20, 3)), _batch(8, 8, P=20))
    finally:
        config.set_active_cfg(cfg)
    cfg3 = config.default_cfg()
    cfg3.skip_eval = True
    assert make_evaluator(cfg3) is None
    assert len(ev) == 0

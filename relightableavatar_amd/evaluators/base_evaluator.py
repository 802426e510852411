"""Device-side mirror of the reference's evaluator: MSE, PSNR, SSIM and LPIPS of a rendered frame against the ground truth.

    Evaluator.evaluate(output, batch), Evaluator.summarize()      lib/evaluators/base_evaluator.py:71-129
    cfg.eval_whole_img                                            lib/config/config.py:215

evaluate() queues one ra_image_metrics call per frame (Engine.image_metrics) into a growing device table and reads nothing back;
summarize() does the only device-to-host copies, returns the means, keeps the per-frame lists in self.metrics (what the reference
saves as metrics.npy) and resets the evaluator.  There is no CPU fallback.

When the engine holds an LPIPS weight set (Engine.lpips_load), evaluate() also queues one ra_lpips call per frame (Engine.lpips) into a
second growing table, and summarize() returns a fourth key 'lpips'.  Without a loaded set nothing changes: three keys, no extra call.

Scope, stated rather than implied:
  - LPIPS (:19-24, 50-69, 103-104) is lpips.LPIPS() at its defaults on the [0, 1] images, as the reference calls it (no normalize=True),
    assembled and cropped like the SSIM's.  Its pretrained weights are NOT part of this project: the user loads a state dict
    (INTEGRATION.md).  Without one summarize() has no 'lpips' key — not a silent zero.  Frames evaluated before the weights were loaded
    and frames after them must not be mixed in one summary: summarize() refuses unequal counts.
  - Writing images (self.visualize, the metrics.npy file) stays out, as in the visualiser.
  - A batch with crop_bbox is refused: the reference's own two-argument fill_image call (:41-43) raises a TypeError there, so there is
    nothing to mirror.
  - cfg.eval_whole_img = False on a ray list (P != H*W) is refused: the reference slices the (P, 3) ray list by an image rectangle
    there (:38-39) and scores a one-dimensional signal.  On H*W rays it is supported: mse and psnr over the rays (which are all
    pixels), ssim on cv2.boundingRect(mask_at_box).
  - A device-resident mask_at_box is not counted (that would be a read-back): a ray beyond the mask's nonzero pixels is dropped, a
    nonzero pixel beyond the rays keeps the background.  A host mask whose count differs from P is refused.
"""
import numpy as np
import torch

from .. import config


class Evaluator:
    engine = None      # the Engine that owns the HIP context (set once: Evaluator.engine = net.engine())
    GROW = 64          # rows the table grows by

    def __init__(self):
        self.metrics = None      # the per-frame lists of the last summary
        self._table = None
        self._n = 0
        self._lpips = None       # the second table: (N, 6) [lpips, r_0 .. r_4] per frame, filled while the engine holds LPIPS weights
        self._n_lpips = 0

    def __len__(self):
        return self._n

    def _row(self, dev):
        if self._table is None or self._n == self._table.shape[0]:
            grown = torch.empty(self._n + self.GROW, 4, dtype=torch.float64, device=dev)
            if self._n:
                grown[:self._n].copy_(self._table)          # on the stream, behind the calls that filled it
            self._table = grown
        self._n += 1
        return self._table[self._n - 1]

    def _lpips_row(self, dev):
        if self._lpips is None or self._n_lpips == self._lpips.shape[0]:
            grown = torch.empty(self._n_lpips + self.GROW, 6, dtype=torch.float64, device=dev)
            if self._n_lpips:
                grown[:self._n_lpips].copy_(self._lpips)
            self._lpips = grown
        self._n_lpips += 1
        return self._lpips[self._n_lpips - 1]

    def evaluate(self, output, batch, engine=None):
        cfg = config.active_cfg()
        if 'crop_bbox' in batch:
            raise NotImplementedError('Evaluator.evaluate: a batch with crop_bbox is not supported: the reference\'s own fill_image call '
                                      '(base_evaluator.py:41-43) raises a TypeError, there is nothing to mirror')
        H, W = int(batch['meta']['H'].item()), int(batch['meta']['W'].item())
        pred, gt = output['rgb_map'][0], batch['rgb'][0]
        if pred.ndim == 3:                                    # :86-88: the maps are images already
            pred, gt = pred.reshape(-1, 3), gt.reshape(-1, 3)
        P = pred.shape[0]
        if tuple(pred.shape) != (P, 3) or tuple(gt.shape) != (P, 3):
            raise ValueError(f'Evaluator.evaluate: rgb_map {tuple(pred.shape)} and batch.rgb {tuple(gt.shape)} must both be (P, 3)')
        whole = bool(cfg.get('eval_whole_img', True))
        if not whole and P != H * W:
            raise NotImplementedError('cfg.eval_whole_img = False on a ray list is not supported: the reference slices the (P, 3) ray list by '
                                      'an image rectangle (base_evaluator.py:38-39) and scores a one-dimensional signal')
        mask = None
        if P != H * W or not whole:
            mask = batch['mask_at_box'][0].reshape(-1)
            if mask.numel() != H * W:
                raise ValueError(f'Evaluator.evaluate: mask_at_box has {mask.numel()} entries, the image {H * W}')
            if not mask.is_cuda and P != H * W and int(mask.ne(0).sum()) != P:
                raise ValueError(f'Evaluator.evaluate: mask_at_box selects {int(mask.ne(0).sum())} pixels, rgb_map has {P} rays')
        eng = engine or Evaluator.engine
        if eng is None:
            raise RuntimeError('Evaluator.evaluate needs the engine of the network (Evaluator.engine = net.engine()); no CPU fallback')
        dev = eng.device
        pix = None
        if P != H * W:                                        # mask_at_box.nonzero() without its read-back of the count
            m = mask.to(dev).ne(0)
            rank = torch.cumsum(m, 0) - 1
            pix = torch.full((P + 1,), -1, dtype=torch.int64, device=dev)
            pix.scatter_(0, torch.where(m & (rank < P), rank, torch.full_like(rank, P)), torch.arange(H * W, device=dev))
            pix = pix[:P]
        eng.image_metrics(pred, gt, H, W, pix=pix, mask=None if whole else mask, bg=float(cfg.bg_brightness), mse_over_rays=not whole,
                          out=self._row(dev))
        if eng.lpips_loaded():
            eng.lpips(pred, gt, H, W, pix=pix, mask=None if whole else mask, bg=float(cfg.bg_brightness), out=self._lpips_row(dev))

    def summarize(self):
        if self._n == 0:
            raise RuntimeError('Evaluator.summarize: no frame was evaluated')
        if self._n_lpips not in (0, self._n):
            raise RuntimeError(f'Evaluator.summarize: {self._n} frames but {self._n_lpips} with LPIPS: the weights were loaded between frames')
        rows = self._table[:self._n].cpu().numpy()            # the one device-to-host copy
        self.metrics = {'mse': rows[:, 0].tolist(), 'psnr': rows[:, 1].tolist(), 'ssim': rows[:, 2].tolist()}      # the reference's metrics.npy
        if self._n_lpips:
            self.metrics['lpips'] = self._lpips[:self._n_lpips, 0].cpu().numpy().tolist()      # ... and one more with LPIPS weights loaded
        self._table, self._n, self._lpips, self._n_lpips = None, 0, None, 0
        return {k: float(np.mean(v)) for k, v in self.metrics.items()}

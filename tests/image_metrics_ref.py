"""Host restatements of the evaluator's metrics (helper of test_oracle_image_metrics.py / test_gpu_image_metrics.py; not a test).

Three evaluations of ONE formula — skimage.metrics.structural_similarity(pred, gt, channel_axis=-1, data_range=1) at its defaults
(7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, 3 border pixels cropped) and mean((pred - gt)^2), -10 log10(mse):
    truth(...)                  (a) direct sums over the valid windows in np.longdouble (the variances as centred sums: no cancellation)
    restated(..., np.float64)   (b) what scikit-image does: scipy.ndimage.uniform_filter(size=7) of x, y, x^2, y^2, xy, crop 3, mean
    restated(..., np.float32)   (c) the same in float32 — scikit-image's own arithmetic for the float32 images the reference hands it

No fixture made by the reference is possible: skimage, cv2 and lpips are not installed where this project is built, so the reference's
evaluator cannot be imported; (b) restates scikit-image's published algorithm on scipy, which is installed.
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN, NP_, K1, K2 = 7, 49, 0.01, 0.03
U = 2.0 ** -53            # unit roundoff of double

SIZES = [(7, 7), (7, 9), (8, 8), (33, 70), (37, 39), (39, 38), (64, 64), (256, 300)]       # 38 pixels = one 32-window tile: one short, one past
SETS = ('noise', 'smooth', 'sparse')


def box_of(H, W):
    """the 24 x 16 box of `sparse` (rows x columns), shrunk to the image where it does not fit: y0, x0, h, w"""
    h, w = min(24, H), min(16, W)
    return (H - h) // 2, (W - w) // 3, h, w


def make_set(name, H, W):
    """-> pred, gt: (H, W, 3) float32 in [0, 1]"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if name == 'noise':
        gt = rng.uniform(size=(H, W, 3))
        pred = np.clip(gt + 0.05 * rng.standard_normal((H, W, 3)), 0, 1)
    elif name == 'smooth':
        pred = np.stack([0.5 + 0.4 * np.sin(xx / 9 + c) * np.cos(yy / 7) for c in range(3)], -1)
        gt = 0.98 * pred + 0.01
    elif name == 'sparse':
        y0, x0, h, w = box_of(H, W)
        gt, pred = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        tex = rng.uniform(0.2, 0.9, size=(h, w, 3))
        gt[y0:y0 + h, x0:x0 + w] = tex
        pred[y0:y0 + h, x0:x0 + w] = np.clip(tex + 0.03 * rng.standard_normal((h, w, 3)), 0, 1)
    else:
        raise KeyError(name)
    return pred.astype(np.float32), gt.astype(np.float32)


def mse_psnr(pred, gt, dtype=np.longdouble):
    d = pred.astype(dtype) - gt.astype(dtype)
    mse = np.mean(d * d, dtype=dtype)
    with np.errstate(divide='ignore'):
        return mse, -10 * np.log10(mse)


def truth(pred, gt, data_range=1.0):
    """(a) -> dict(mse, psnr, ssim, windows) in longdouble; ssim NaN and windows 0 where skimage raises (a side below 7)"""
    L = np.longdouble
    mse, psnr = mse_psnr(pred, gt, L)
    H, W = pred.shape[:2]
    if H < WIN or W < WIN:
        return dict(mse=mse, psnr=psnr, ssim=L('nan'), windows=0)
    h, w = H - WIN + 1, W - WIN + 1
    x, y = pred.astype(L), gt.astype(L)
    shifts = [(dy, dx) for dy in range(WIN) for dx in range(WIN)]
    ux, uy = sum(x[dy:dy + h, dx:dx + w] for dy, dx in shifts) / NP_, sum(y[dy:dy + h, dx:dx + w] for dy, dx in shifts) / NP_
    vx = sum((x[dy:dy + h, dx:dx + w] - ux) ** 2 for dy, dx in shifts) / (NP_ - 1)
    vy = sum((y[dy:dy + h, dx:dx + w] - uy) ** 2 for dy, dx in shifts) / (NP_ - 1)
    vxy = sum((x[dy:dy + h, dx:dx + w] - ux) * (y[dy:dy + h, dx:dx + w] - uy) for dy, dx in shifts) / (NP_ - 1)
    c1, c2 = (L(K1) * L(data_range)) ** 2, (L(K2) * L(data_range)) ** 2
    S = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return dict(mse=mse, psnr=psnr, ssim=S.mean(axis=(0, 1), dtype=L).mean(dtype=L), windows=h * w)


def restated(pred, gt, dtype=np.float64, data_range=1.0):
    """(b) / (c): scikit-image's structural_similarity on scipy, per channel, in dtype (its float32 path keeps float32 images as they are)"""
    mse, psnr = mse_psnr(pred, gt, dtype)
    H, W = pred.shape[:2]
    if H < WIN or W < WIN:
        return dict(mse=mse, psnr=psnr, ssim=dtype('nan'), windows=0)
    c1, c2, cov_norm = (K1 * data_range) ** 2, (K2 * data_range) ** 2, NP_ / (NP_ - 1)
    per_channel = []
    for ch in range(pred.shape[2]):
        x, y = pred[..., ch].astype(dtype), gt[..., ch].astype(dtype)
        ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
        uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        pad = (WIN - 1) // 2
        per_channel.append(S[pad:H - pad, pad:W - pad].mean(dtype=np.float64))
    return dict(mse=mse, psnr=psnr, ssim=np.mean(per_channel), windows=(H - WIN + 1) * (W - WIN + 1))


def bounding_rect(mask):
    """cv2.boundingRect of the nonzero pixels of an (H, W) mask: x, y, w, h (zeros for an empty mask)"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def assemble(rays, pix, H, W, bg):
    """base_evaluator.py:81-85: the (P, 3) rays scattered over a bg image, in float32 like the inputs"""
    img = np.full((H * W, 3), bg, np.float32)
    img[pix] = rays
    return img.reshape(H, W, 3)


def dist(v, t):
    """distance of a value from the truth; 0 where both are the same infinity or both NaN"""
    v, t = np.longdouble(v), np.longdouble(t)
    if (np.isnan(v) and np.isnan(t)) or (np.isinf(t) and v == t):
        return np.longdouble(0)
    return abs(v - t)


def allowed(b, t):
    """the parity rule (section 12's, one precision up): at most 10 x the float64 restatement's own distance from
    the truth, or 8 double unit roundoffs of the value where that is larger"""
    return max(10 * dist(b, t), 8 * U * abs(np.longdouble(t)))

"""Host restatements of LPIPS (AlexNet, version 0.1) as the reference's evaluator calls it (helper of test_oracle_lpips.py /
test_gpu_lpips.py; not a test).  Neither `lpips` nor `torchvision` is installed where this project is built, so the specification is
restated here — three evaluations of ONE spec (include/relightableavatar.h):

    lpips(..., torch.float64)   (a) truth: torch.nn.functional.conv2d / max_pool2d in float64 on the fp32 inputs and fp32 weights
    lpips(..., torch.float32)   (b) the same in float32 — what the reference's own arithmetic does
    lpips_loops(...)            (c) an independent numpy float64 evaluation by direct loops over the output positions, sharing no code
                                    with (a); used at 31 x 31 only

    x = (x - shift) / scale; conv 11/4/2 3->64, ReLU [tap 0], maxpool 3/2, conv 5/1/2 64->192, ReLU [1], maxpool 3/2, conv 3/1/1 192->384,
    ReLU [2], conv 3/1/1 384->256, ReLU [3], conv 3/1/1 256->256, ReLU [4]; per tap n = f / (sqrt(sum_c f^2) + 1e-10),
    r_k = mean over positions of sum_c lin_k[c] (n0 - n1)^2; value = r_0 + ... + r_4.  Images are in [0, 1]: no 2x - 1.

The weights are synthetic (seeded): the metric is a fixed architecture applied to a user-supplied state dict.
"""
import numpy as np
import torch
import torch.nn.functional as F

import image_metrics_ref as IM

U32 = 2.0 ** -24          # unit roundoff of float32
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))      # Cin, Cout, k, stride, pad
POOL_BEFORE = (False, True, True, False, False)
MIN_SIDE = 31
SETS = ('noise', 'smooth', 'sparse', 'inverse')
SIZES = [(31, 31), (31, 34), (32, 47), (35, 35), (39, 39), (64, 64), (67, 130), (256, 300)]


def make_weights(seed=0):
    """neutral-layout state dict: conv weights N(0, 2 / (Cin k k)), biases N(0, 0.05^2), lin weights U(0, 2 / C) (non-negative like the
    trained ones), all float32"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, (cin, cout, ks, _, _) in enumerate(CONVS):
        sd[f'conv{k}.weight'] = (torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * (2.0 / (cin * ks * ks)) ** 0.5).float()
        sd[f'conv{k}.bias'] = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.05).float()
    for k, (_, cout, _, _, _) in enumerate(CONVS):
        sd[f'lin{k}.weight'] = (torch.rand(1, cout, 1, 1, generator=g, dtype=torch.float64) * (2.0 / cout)).float()
    return sd


def make_set(name, H, W):
    """-> x0, x1: (H, W, 3) float32 in [0, 1]; the first three are section 14's sets, `inverse` is x against 1 - x"""
    if name == 'inverse':
        x = IM.make_set('noise', H, W)[1]
        return x, (np.float32(1) - x).astype(np.float32)
    return IM.make_set(name, H, W)


def tap_sizes(H, W):
    """the (h, w) of the five taps by the spec's formulas; None below 31 in a dimension (torch raises in the second pool)"""
    if H < MIN_SIDE or W < MIN_SIDE:
        return None
    conv = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    pool = lambda n: (n - 3) // 2 + 1
    h, w, out = H, W, []
    for (cin, cout, ks, st, pad), pb in zip(CONVS, POOL_BEFORE):
        if pb:
            h, w = pool(h), pool(w)
        h, w = conv(h, ks, st, pad), conv(w, ks, st, pad)
        out.append((h, w))
    return out


def features(img, sd, dtype):
    """img (H, W, 3) float32 -> the five post-ReLU taps as (C, h, w) tensors of dtype"""
    x = torch.tensor(img).permute(2, 0, 1)[None].to(dtype)          # a copy: the shared cases are read-only
    shift = torch.tensor(sd.get('shift', SHIFT), dtype=torch.float32).reshape(1, 3, 1, 1).to(dtype)
    scale = torch.tensor(sd.get('scale', SCALE), dtype=torch.float32).reshape(1, 3, 1, 1).to(dtype)
    x = (x - shift) / scale
    taps = []
    for k, ((cin, cout, ks, st, pad), pb) in enumerate(zip(CONVS, POOL_BEFORE)):
        if pb:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[f'conv{k}.weight'].to(dtype), sd[f'conv{k}.bias'].to(dtype), stride=st, padding=pad))
        taps.append(x[0])
    return taps


def lpips_of_taps(t0, t1, sd):
    """[value, r_0 .. r_4] in the taps' dtype"""
    dtype = t0[0].dtype
    r = []
    for k, (a, b) in enumerate(zip(t0, t1)):
        na = a / (torch.sqrt(torch.sum(a * a, dim=0, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b * b, dim=0, keepdim=True)) + 1e-10)
        d = (na - nb) ** 2
        r.append((d * sd[f'lin{k}.weight'].to(dtype).reshape(-1, 1, 1)).sum(dim=0).mean())
    total = r[0]
    for v in r[1:]:
        total = total + v
    return torch.stack([total] + r)


def lpips(x0, x1, sd, dtype=torch.float64):
    """-> (six values as float64 numpy, taps of x0, taps of x1); six NaNs (and no taps) below 31 in a dimension"""
    if tap_sizes(*x0.shape[:2]) is None:
        return np.full(6, np.nan), None, None
    with torch.no_grad():
        t0, t1 = features(x0, sd, dtype), features(x1, sd, dtype)
        return lpips_of_taps(t0, t1, sd).double().numpy(), t0, t1


def _conv_loops(x, w, b, stride, pad):
    """x (C, h, w), w (Cout, C, k, k) float64: one output position at a time"""
    c, h, wd = x.shape
    k = w.shape[2]
    xp = np.zeros((c, h + 2 * pad, wd + 2 * pad))
    xp[:, pad:pad + h, pad:pad + wd] = x
    oh, ow = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    out = np.empty((w.shape[0], oh, ow))
    for i in range(oh):
        for j in range(ow):
            patch = xp[:, i * stride:i * stride + k, j * stride:j * stride + k]
            out[:, i, j] = np.maximum((w * patch[None]).sum(axis=(1, 2, 3)) + b, 0.0)
    return out


def _pool_loops(x):
    c, h, w = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = np.empty((c, oh, ow))
    for i in range(oh):
        for j in range(ow):
            out[:, i, j] = x[:, 2 * i:2 * i + 3, 2 * j:2 * j + 3].reshape(c, -1).max(axis=1)
    return out


def lpips_loops(x0, x1, sd):
    """(c): numpy float64, loops; -> six values"""
    shift, scale = np.asarray(SHIFT, np.float32).astype(np.float64), np.asarray(SCALE, np.float32).astype(np.float64)
    taps = []
    for img in (x0, x1):
        x = (img.astype(np.float64).transpose(2, 0, 1) - shift[:, None, None]) / scale[:, None, None]
        mine = []
        for k, ((cin, cout, ks, st, pad), pb) in enumerate(zip(CONVS, POOL_BEFORE)):
            if pb:
                x = _pool_loops(x)
            x = _conv_loops(x, sd[f'conv{k}.weight'].double().numpy(), sd[f'conv{k}.bias'].double().numpy(), st, pad)
            mine.append(x)
        taps.append(mine)
    r = []
    for k in range(5):
        a, b = taps[0][k], taps[1][k]
        lin = sd[f'lin{k}.weight'].double().numpy().reshape(-1)
        acc = 0.0
        for i in range(a.shape[1]):
            for j in range(a.shape[2]):
                na = a[:, i, j] / (np.sqrt(np.sum(a[:, i, j] ** 2)) + 1e-10)
                nb = b[:, i, j] / (np.sqrt(np.sum(b[:, i, j] ** 2)) + 1e-10)
                acc += float(np.sum(lin * (na - nb) ** 2))
        r.append(acc / (a.shape[1] * a.shape[2]))
    return np.array([sum(r)] + r)


def allowed(b, t):
    """the parity rule for the six outputs (the project's 10 x float32 rule, no new constant): at most 10 x the float32 restatement's own
    distance from the truth, or 8 float32 unit roundoffs of the value where that is larger (a scalar's fp32 error can be small by luck)"""
    return max(10 * IM.dist(b, t), 8 * U32 * abs(np.longdouble(t)))


_cache = {}


def case(name, H, W, seed=0):
    """x0, x1, truth (6,), float32 restatement (6,), truth taps of x0, float32 taps of x0 — computed once per process, read-only"""
    key = (name, H, W, seed)
    if key not in _cache:
        x0, x1 = make_set(name, H, W)
        x0.setflags(write=False), x1.setflags(write=False)
        sd = weights(seed)
        t, t0, _ = lpips(x0, x1, sd, torch.float64)
        b, b0, _ = lpips(x0, x1, sd, torch.float32)
        _cache[key] = (x0, x1, t, b, t0, b0)
    return _cache[key]


def weights(seed=0):
    key = ('weights', seed)
    if key not in _cache:
        _cache[key] = make_weights(seed)
    return _cache[key]

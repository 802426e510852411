"""Restatements of the texture path's rule (relightableavatar_amd/csrc/ra_texture_rules.hpp) for the tests.

  rast_db(pos, faces, face_map, H, W, dt), attr_da(...)    the pixel differentials, in float32 kernel order or in float64
  mips(tex, max_mip_level, dt)                             the chain, ((a + b) + (c + d)) 0.25
  log2_poly(x)                                             the header's log2 in numpy float32: what the device must equal bit for bit
  pixel(uv, uv_da, ..., dt, log2)                          what a pixel decides: ok, the level pair, f, the taps and weights.  dt = float32
                                                           with log2 = 'poly' is the kernel's; float64 with log2 = 'true' the reference;
                                                           float32 with log2 = 'numpy' the plain baseline of the 10 x rule
  forward(tex, px, dt), duv_closed(...), dtex_closed(...)  the output and the closed-form gradients in either precision
  dtex_kernel_order(...)                                   the backward kernels' float32 operations in their order: one wave per (view, level,
                                                           texel) run, lane stride 64 and xor tree (raster_ref._wave_sum), the fold, the views
  texture_torch(tex, uv, px)                               torch float64 with the cells, the level pair and f of px held fixed, for autograd
  undecided(px32, px64)                                    pixels where the two precisions choose another texel cell at a used level or another l0
  CASES, case(name), reference(name, filt, boundary)       the case table and the shared, read-only references
  render_reference(H, W, R_S), fit_inputs(), fit_float64() render_textured's texture branch in float64 and plain float32; the end-to-end fit
The inputs are float32; every restatement starts from the same float32 values.
"""
import functools

import numpy as np

import raster_ref as R
from antialias_ref import UNDECIDED_CAP  # noqa: F401  (the cap on the share of undecided pixels: a condition, not a measurement)

NEAREST, LINEAR, TRILINEAR = 'nearest', 'linear', 'linear-mipmap-linear'
FILTERS, BOUNDARIES = (NEAREST, LINEAR, TRILINEAR), ('wrap', 'clamp')
TAPS = {NEAREST: 1, LINEAR: 4, TRILINEAR: 8}
MAX_LEVELS, MAX_CHANNELS = 16, 64
f32 = np.float32
SQRT2 = f32('1.41421354')
K1, K3, K5, K7, K9 = (f32(s) for s in ('2.88539004', '0.961796701', '0.577078044', '0.412198603', '0.320598900'))


# ---- pixel differentials ----------------------------------------------------------------------------------------------------------------
def rast_db(pos, faces, face_map, H, W, dt=np.float32):
    """(B,H,W,4): (du/dX, du/dY, dv/dX, dv/dY) of the face each pixel holds, 0 where it is empty; texture_db's operations in its order"""
    pos = pos[None] if pos.ndim == 2 else pos
    B = pos.shape[0]
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    px, py = R.centre(ix, W, dt), R.centre(iy, H, dt)
    out = np.zeros((B, H, W, 4), dt)
    scale = (dt(2) / dt(W), dt(2) / dt(H))
    with np.errstate(all='ignore'):
        for b in range(B):
            for f in np.unique(face_map[b][face_map[b] >= 0]):
                idx = faces[f]
                m = face_map[b] == f
                i0, i1, i2 = (int(i) for i in idx)
                p = [pos[b, i].astype(dt) for i in idx]
                c, neg = np.zeros((3, 3), dt), np.zeros(3, bool)
                for k, (ia, ib, a, bb) in enumerate(((i1, i2, p[1], p[2]), (i2, i0, p[2], p[0]), (i0, i1, p[0], p[1]))):
                    if ia < ib:
                        c[k] = R._edge(a, bb, dt)
                    else:
                        c[k], neg[k] = R._edge(bb, a, dt), True
                x, y = px[m], py[m]
                E = [(c[k, 0] * x + c[k, 1] * y) + c[k, 2] for k in range(3)]
                e = [-E[k] if neg[k] else E[k] for k in range(3)]
                S = (e[0] + e[1]) + e[2]
                b0, b1 = e[0] / S, e[1] / S
                o = np.zeros((len(x), 4), dt)
                for a in range(2):
                    cs = [-c[k, a] if neg[k] else c[k, a] for k in range(3)]
                    tot = (cs[0] + cs[1]) + cs[2]
                    o[:, a] = ((cs[0] - b0 * tot) / S) * scale[a]
                    o[:, 2 + a] = ((cs[1] - b1 * tot) / S) * scale[a]
                out[b][m] = o
    return out


def attr_da(attr, faces, face_map, db, channels, dt=np.float32):
    """(B,H,W,2n): (da/dX, da/dY) of the selected channels, texture_attr_da's operations"""
    B, H, W = face_map.shape
    a = np.broadcast_to(attr, (B,) + attr.shape[-2:]).astype(dt)
    db = db.astype(dt)
    out = np.zeros((B, H, W, 2 * len(channels)), dt)
    for b in range(B):
        got = face_map[b] >= 0
        corner = a[b][faces[np.maximum(face_map[b], 0)]]          # (H,W,3,A)
        for k, ch in enumerate(channels):
            d0, d1 = corner[..., 0, ch] - corner[..., 2, ch], corner[..., 1, ch] - corner[..., 2, ch]
            out[b, ..., 2 * k] = np.where(got, db[b, ..., 0] * d0 + db[b, ..., 2] * d1, 0)
            out[b, ..., 2 * k + 1] = np.where(got, db[b, ..., 1] * d0 + db[b, ..., 3] * d1, 0)
    return out


def bary64(pos, idx, px, py):
    """(u, v) of one face at the float64 sample points, for the central differences"""
    rec = R.setup([pos[i] for i in idx], idx, 1, 1, np.float64, box=False)
    c, neg = rec[0], rec[1]
    e = [(-1 if neg[k] else 1) * ((c[k, 0] * px + c[k, 1] * py) + c[k, 2]) for k in range(3)]
    S = (e[0] + e[1]) + e[2]
    return e[0] / S, e[1] / S


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
def levels(TH, TW, max_mip_level):
    """(heights, widths, offsets in texels; offsets[-1] is the chain's size)"""
    hs, ws = [TH], [TW]
    while len(hs) - 1 < max_mip_level and len(hs) < MAX_LEVELS:
        h, w = hs[-1], ws[-1]
        if w < 2 or h < 2 or (w & 1) or (h & 1):
            break
        hs.append(h // 2)
        ws.append(w // 2)
    off = np.concatenate([[0], np.cumsum([h * w for h, w in zip(hs, ws)])]).astype(np.int64)
    return hs, ws, off


def mips(tex, max_mip_level, dt=np.float32):
    """tex (Bt,TH,TW,C) -> the list of levels (Bt,h,w,C) in dt"""
    hs, _, _ = levels(tex.shape[1], tex.shape[2], max_mip_level)
    out = [tex.astype(dt)]
    for _ in hs[1:]:
        s = out[-1]
        a, b, c, d = s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2]
        out.append(((a + b) + (c + d)) * dt(0.25))
    return out


def flat_chain(chain):
    """the levels side by side: (Bt, texels of the chain, C)"""
    return np.concatenate([l.reshape(l.shape[0], -1, l.shape[-1]) for l in chain], axis=1)


# ---- log2 and the level of detail -------------------------------------------------------------------------------------------------------
def log2_poly(x):
    """texture_log2 on a float32 array of normal positive values, one numpy float32 operation per rounding"""
    x = np.ascontiguousarray(x, f32)
    bits = x.view(np.uint32)
    e = ((bits >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32) - 127
    m = ((bits & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(f32)
    big = m > SQRT2
    m = np.where(big, m * f32(0.5), m)
    e = e + big
    num, den = m - f32(1), m + f32(1)
    s = num / den
    z = s * s
    p = K9 * z
    p = p + K7
    p = p * z
    p = p + K5
    p = p * z
    p = p + K3
    p = p * z
    p = p + K1
    return e.astype(f32) + s * p


def lod(da, TH, TW, Lmax, dt, log2):
    """(l0 int, f dt) per pixel; log2: 'poly' (the header's, float32 only), 'numpy' (numpy's own in dt: the plain baseline and the float64 truth)"""
    da = da.astype(dt)
    with np.errstate(all='ignore'):
        ax, ay, bx, by = da[..., 0] * dt(TW), da[..., 1] * dt(TW), da[..., 2] * dt(TH), da[..., 3] * dt(TH)
        A, Bq, Cq = ax * ax + ay * ay, bx * bx + by * by, ax * bx + ay * by
        h = dt(0.5) * (A + Bq)
        d = A - Bq
        m2 = h + np.sqrt(dt(0.25) * (d * d) + Cq * Cq)
        l0, f = np.zeros(m2.shape, np.int64), np.zeros(m2.shape, dt)
        live = m2 > 1
        huge = live & ~(m2 < dt(f32(3.0e38)))
        mid = live & ~huge
        lg = np.zeros(m2.shape, dt)
        lg[mid] = log2_poly(m2[mid]) if log2 == 'poly' else np.log2(m2[mid])
        lv = dt(0.5) * lg
        top = huge | (mid & ~(lv < dt(Lmax)))
        inner = mid & ~top
        fl = np.floor(lv)
        l0[top] = Lmax
        l0[inner] = fl[inner].astype(np.int64)
        f[inner] = (lv - fl)[inner]
    return l0, f


# ---- a pixel ------------------------------------------------------------------------------------------------------------------------------
def _index(i, n, boundary):
    return np.clip(i, 0, n - 1) if boundary == 'clamp' else np.mod(i, n)


def pixel(uv, uv_da, TH, TW, filt, boundary, max_mip_level, dt=np.float32, log2='poly'):
    """what texture_pixel decides for every pixel of uv (B,H,W,2): dict(ok, l0, two, f, lev (2,...) the level of each half, gidx (2,4,...)
    the taps' texels in the flat chain, w (2,4,...) their weights, fx, fy, gx, gy (2,...), cell (2,2,...) the unwrapped (x0, y0), ext (2,2,...) the
    (w, h) of each half's level, hs, ws, off).  nearest: gidx[0, 0] and cell[0] alone."""
    hs, ws, off = levels(TH, TW, max_mip_level if filt == TRILINEAR else 0)
    Lmax = len(hs) - 1
    hs_a, ws_a = np.asarray(hs), np.asarray(ws)
    u, v = uv[..., 0].astype(dt), uv[..., 1].astype(dt)
    shape = u.shape
    with np.errstate(all='ignore'):
        ok = (np.abs(u * dt(TW)) < 2.0 ** 30) & (np.abs(v * dt(TH)) < 2.0 ** 30)
        l0, f = np.zeros(shape, np.int64), np.zeros(shape, dt)
        if filt == TRILINEAR:
            l0, f = lod(uv_da, TH, TW, Lmax, dt, log2)
        two = ok & (f != 0)
        us, vs = np.where(ok, u, 0), np.where(ok, v, 0)
        px = dict(ok=ok, l0=l0, two=two, f=f, hs=hs, ws=ws, off=off, filt=filt, boundary=boundary, dt=dt)
        if filt == NEAREST:
            cx, cy = np.floor(us * dt(TW)).astype(np.int64), np.floor(vs * dt(TH)).astype(np.int64)
            g = _index(cy, TH, boundary) * TW + _index(cx, TW, boundary)
            px.update(gidx=g[None, None], cell=np.stack([cx, cy])[None], lev=np.zeros((1,) + shape, np.int64))
            return px
        lev = np.stack([l0, np.minimum(l0 + 1, Lmax)])
        keys = dict(gidx=[], w=[], fx=[], fy=[], gx=[], gy=[], cell=[], ext=[])
        for k in range(2):
            wl, hl = ws_a[lev[k]], hs_a[lev[k]]
            x, y = us * wl.astype(dt) - dt(0.5), vs * hl.astype(dt) - dt(0.5)
            flx, fly = np.floor(x), np.floor(y)
            fx, fy = x - flx, y - fly
            ixx, iyy = flx.astype(np.int64), fly.astype(np.int64)
            x0, x1, y0, y1 = _index(ixx, wl, boundary), _index(ixx + 1, wl, boundary), _index(iyy, hl, boundary), _index(iyy + 1, hl, boundary)
            gx, gy = dt(1) - fx, dt(1) - fy
            base = off[lev[k]]
            keys['gidx'].append(np.stack([base + y0 * wl + x0, base + y0 * wl + x1, base + y1 * wl + x0, base + y1 * wl + x1]))
            keys['w'].append(np.stack([gx * gy, fx * gy, gx * fy, fx * fy]))
            for name, val in (('fx', fx), ('fy', fy), ('gx', gx), ('gy', gy), ('cell', np.stack([ixx, iyy])), ('ext', np.stack([wl, hl]))):
                keys[name].append(val)
        px.update({name: np.stack(val) for name, val in keys.items()}, lev=lev)
    return px


def _texels(flat, px, b, k):
    """the four taps of half k of view b: (4, H, W, C)"""
    bt = 0 if flat.shape[0] == 1 else b
    return flat[bt][px['gidx'][k][:, b]]


def forward(tex, px, max_mip_level, dt=np.float32):
    """out (B,H,W,C) in dt: texture_value's operations in its order"""
    filt = px['filt']
    flat = flat_chain(mips(tex, max_mip_level if filt == TRILINEAR else 0, dt))
    B, H, W = px['ok'].shape
    out = np.zeros((B, H, W, tex.shape[-1]), dt)
    with np.errstate(all='ignore'):
        for b in range(B):
            ok = px['ok'][b][..., None]
            if filt == NEAREST:
                out[b] = np.where(ok, flat[0 if flat.shape[0] == 1 else b][px['gidx'][0, 0, b]], 0)
                continue
            v = []
            for k in range(2):
                t, w = _texels(flat, px, b, k), px['w'][k][:, b][..., None]
                v.append(((w[0] * t[0] + w[1] * t[1]) + w[2] * t[2]) + w[3] * t[3])
            f = px['f'][b][..., None]
            mixed = (dt(1) - f) * v[0] + f * v[1]
            out[b] = np.where(ok, np.where(px['two'][b][..., None], mixed, v[0]), 0)
    return out


def duv_closed(tex, px, dout, max_mip_level, dt=np.float32):
    """duv (B,H,W,2) in dt: texture_duv's operations in its order (the channels ascending, the extent, the two levels mixed)"""
    filt = px['filt']
    B, H, W = px['ok'].shape
    out = np.zeros((B, H, W, 2), dt)
    if filt == NEAREST:
        return out
    flat = flat_chain(mips(tex, max_mip_level if filt == TRILINEAR else 0, dt))
    d = dout.astype(dt)
    with np.errstate(all='ignore'):
        for b in range(B):
            U, V = [], []
            for k in range(2):
                t = _texels(flat, px, b, k)
                fx, fy, gx, gy = (px[n][k][b] for n in ('fx', 'fy', 'gx', 'gy'))
                su, sv = np.zeros((H, W), dt), np.zeros((H, W), dt)
                for c in range(tex.shape[-1]):
                    t0, t1, t2, t3 = (t[q][..., c] for q in range(4))
                    du = (t1 - t0) * gy + (t3 - t2) * fy
                    dv = (t2 - t0) * gx + (t3 - t1) * fx
                    su = su + d[b, ..., c] * du
                    sv = sv + d[b, ..., c] * dv
                U.append(su * px['ext'][k][0][b].astype(dt))
                V.append(sv * px['ext'][k][1][b].astype(dt))
            f, two, ok = px['f'][b], px['two'][b], px['ok'][b]
            g = dt(1) - f
            out[b, ..., 0] = np.where(ok, np.where(two, g * U[0] + f * U[1], U[0]), 0)
            out[b, ..., 1] = np.where(ok, np.where(two, g * V[0] + f * V[1], V[0]), 0)
    return out


def taps(px, b):
    """the active tap slots of view b in slot order: (group = texel in the flat chain, slot, pixel, weight)"""
    filt, dt = px['filt'], px['dt']
    H, W = px['ok'].shape[1:]
    T = TAPS[filt]
    pix = np.arange(H * W)
    ok = px['ok'][b].reshape(-1)
    if filt == NEAREST:
        return px['gidx'][0, 0, b].reshape(-1)[ok], pix[ok], pix[ok], np.ones(int(ok.sum()), dt)
    group, slot, pixel_, wgt = [], [], [], []
    f = px['f'][b].reshape(-1)
    for k in range(T // 4):
        lw = f if k else dt(1) - f
        act = ok & (px['two'][b].reshape(-1) if k else True)
        for q in range(4):
            group.append(px['gidx'][k][q, b].reshape(-1)[act])
            slot.append((pix * T + 4 * k + q)[act])
            pixel_.append(pix[act])
            wgt.append((lw * px['w'][k][q, b].reshape(-1))[act])
    group, slot, pixel_, wgt = (np.concatenate(a) for a in (group, slot, pixel_, wgt))
    order = np.argsort(slot, kind='stable')
    return group[order], slot[order], pixel_[order], wgt[order]


def run_lengths(px):
    """the number of taps of every (view, level, texel) that has one"""
    out = []
    for b in range(px['ok'].shape[0]):
        n = np.bincount(taps(px, b)[0], minlength=int(px['off'][-1]))
        out.append(n[n > 0])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def _fold(g, px, C):
    """g (texels of the chain, C) of one view -> (TH, TW, C): acc = g_l[y >> l, x >> l] + 0.25 acc from the coarsest level down"""
    hs, ws, off = px['hs'], px['ws'], px['off']
    dt = g.dtype.type
    top = len(hs) - 1
    acc = g[off[top]:off[top + 1]].reshape(hs[top], ws[top], C)
    for l in range(top - 1, -1, -1):
        up = np.repeat(np.repeat(acc, 2, axis=0), 2, axis=1)
        acc = g[off[l]:off[l + 1]].reshape(hs[l], ws[l], C) + dt(0.25) * up
    return acc


def _views(per_view, Bt):
    if Bt != 1:
        return np.stack(per_view)
    s = per_view[0]
    for a in per_view[1:]:
        s = s + a
    return s[None]


def dtex_kernel_order(px, dout, Bt):
    """dtex (Bt,TH,TW,C) float32: texture_run_kernel + texture_fold_kernel restated.  A run is the taps of one (view, level, texel) in slot
    order; lane l adds terms l, l + 64, ... from 0 and the lanes meet in the xor tree (raster_ref._wave_sum); runs of one length are summed
    together, which changes nothing of a run's own order."""
    B = px['ok'].shape[0]
    C = dout.shape[-1]
    d = dout.astype(f32).reshape(B, -1, C)
    per_view = []
    with np.errstate(all='ignore'):
        for b in range(B):
            group, slot, pix, wgt = taps(px, b)
            g = np.zeros((int(px['off'][-1]), C), f32)
            order = np.argsort(group, kind='stable')           # the radix sort: by texel, the slots ascending inside a run
            group, pix, wgt = group[order], pix[order], wgt[order].astype(f32)
            terms = wgt[:, None] * d[b][pix]
            ids, start, count = np.unique(group, return_index=True, return_counts=True)
            for n in np.unique(count):
                sel = count == n
                rows = start[sel][None, :] + np.arange(n)[:, None]          # (n, runs)
                g[ids[sel]] = R._wave_sum(terms[rows])
            per_view.append(_fold(g, px, C))
        return _views(per_view, Bt)


def dtex_closed(px, dout, Bt, dt=np.float64):
    """dtex in dt with no named order (np.add.at), the same taps and fold"""
    B = px['ok'].shape[0]
    C = dout.shape[-1]
    d = dout.astype(dt).reshape(B, -1, C)
    per_view = []
    for b in range(B):
        group, slot, pix, wgt = taps(px, b)
        g = np.zeros((int(px['off'][-1]), C), dt)
        np.add.at(g, group, wgt.astype(dt)[:, None] * d[b][pix])
        per_view.append(_fold(g, px, C))
    return _views(per_view, Bt)


def texture_torch(tex, uv, px, max_mip_level):
    """torch float64: tex (Bt,TH,TW,C) and uv (B,H,W,2) tensors (they may require grad) -> out, with the texel cells, the level pair and f of
    px held fixed — the first-order convention.  The chain is rebuilt in torch, so autograd reaches tex through it."""
    import torch
    filt = px['filt']
    chain = [tex]
    for _ in levels(tex.shape[1], tex.shape[2], max_mip_level if filt == TRILINEAR else 0)[0][1:]:
        s = chain[-1]
        chain.append(((s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])) * 0.25)
    flat = torch.cat([l.reshape(l.shape[0], -1, l.shape[-1]) for l in chain], dim=1)
    B = uv.shape[0]
    ok = torch.as_tensor(px['ok'])[..., None]
    outs = []
    for b in range(B):
        fb = flat[0 if flat.shape[0] == 1 else b]
        if filt == NEAREST:
            outs.append(fb[torch.as_tensor(px['gidx'][0, 0, b])])
            continue
        u, v = torch.where(ok[b, ..., 0], uv[b, ..., 0], 0 * uv[b, ..., 0]), torch.where(ok[b, ..., 0], uv[b, ..., 1], 0 * uv[b, ..., 1])
        val = []
        for k in range(2):
            wl, hl = (torch.as_tensor(px['ext'][k][q][b]).double() for q in range(2))
            fx = u * wl - 0.5 - torch.as_tensor(px['cell'][k][0][b]).double()
            fy = v * hl - 0.5 - torch.as_tensor(px['cell'][k][1][b]).double()
            gx, gy = 1 - fx, 1 - fy
            t = [fb[torch.as_tensor(px['gidx'][k][q, b])] for q in range(4)]
            w = [(gx * gy)[..., None], (fx * gy)[..., None], (gx * fy)[..., None], (fx * fy)[..., None]]
            val.append(w[0] * t[0] + w[1] * t[1] + w[2] * t[2] + w[3] * t[3])
        f = torch.as_tensor(px['f'][b]).double()[..., None]
        outs.append(torch.where(torch.as_tensor(px['two'][b])[..., None], (1 - f) * val[0] + f * val[1], val[0]))
    out = torch.stack(outs)
    return torch.where(ok, out, torch.zeros_like(out))


def undecided(pa, pb):
    """(B,H,W) bool: the two evaluations differ in ok, in l0, in whether the second level is read, or in the texel cell at a level both use"""
    bad = (pa['ok'] != pb['ok']) | (pa['l0'] != pb['l0'])
    if pa['filt'] == NEAREST:
        return bad | (pa['cell'][0] != pb['cell'][0]).any(0)
    bad |= (pa['cell'][0] != pb['cell'][0]).any(0)
    bad |= pa['two'] != pb['two']
    bad |= pa['two'] & pb['two'] & (pa['cell'][1] != pb['cell'][1]).any(0)
    return bad


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# name -> (TH, TW, C, Bt, B, H, W, kind of uv, max_mip_level)
CASE_TABLE = {
    't1x1_c1_1x1': (1, 1, 1, 1, 1, 1, 1, 'random', 8),
    't2x2_c3_9x7': (2, 2, 3, 1, 1, 9, 7, 'random', 8),
    't8x2_c4_9x7_shared3': (8, 2, 4, 1, 3, 9, 7, 'random', 8),              # the chain ends at 4 x 1
    't5x3_c5_9x7_perview3': (5, 3, 5, 3, 3, 9, 7, 'random', 8),            # no mips
    't16_mm8_c3_37x53': (16, 16, 3, 1, 1, 37, 53, 'random', 8),            # the chain clamps at 1 x 1
    't16_mm2_c64_9x7': (16, 16, MAX_CHANNELS, 1, 1, 9, 7, 'random', 2),
    't16_mm8_c3_37x53_perview2': (16, 16, 3, 2, 2, 37, 53, 'random', 8),
    't16_boundary_16x24': (16, 16, 3, 1, 1, 16, 24, 'boundary', 8),        # dyadic uv on texel boundaries, lod on integers, beyond Lmax
    't16_zero_da_9x7': (16, 16, 3, 1, 1, 9, 7, 'zero_da', 8),
    't8x2_runs_7x46': (8, 2, 3, 1, 1, 7, 46, 'runs', 8),                   # nearest: runs of exactly 1, 63, 64, 65, 129 pixels
    't2x2_magnify_64x64': (2, 2, 3, 1, 1, 64, 64, 'magnify', 8),           # runs of over 1 000
}
CASES = tuple(CASE_TABLE)
BY_VALUE = ('t8x2_c4_9x7_shared3', 't5x3_c5_9x7_perview3', 't16_mm8_c3_37x53', 't16_mm8_c3_37x53_perview2', 't16_boundary_16x24', 't2x2_magnify_64x64')
RUN_LENGTHS = (1, 63, 64, 65, 129)


def _freeze(out):
    for a in out.values():
        if isinstance(a, dict):
            _freeze(a)
        elif isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(None)
def case(name):
    """the shared, read-only inputs of one case: tex (Bt,TH,TW,C), uv (B,H,W,2), uv_da (B,H,W,4), dout (B,H,W,C), all float32 and seeded"""
    TH, TW, C, Bt, B, H, W, kind, mm = CASE_TABLE[name]
    rng = np.random.default_rng(R._seed(name))
    tex = rng.standard_normal((Bt, TH, TW, C)).astype(f32)
    dout = rng.standard_normal((B, H, W, C)).astype(f32)
    Lmax = len(levels(TH, TW, mm)[0]) - 1
    if kind in ('random', 'zero_da'):
        uv = rng.uniform(-0.7, 1.9, (B, H, W, 2)).astype(f32)
        spread = 2.0 ** rng.uniform(-2.0, Lmax + 1.5, (B, H, W, 1))
        uv_da = (rng.standard_normal((B, H, W, 4)) * spread / np.array([TW, TW, TH, TH])).astype(f32)
        if kind == 'zero_da':
            uv_da[:] = 0
        if H * W > 2:
            uv[0, 0, 0, 0] = np.nan
            uv[0, -1, -1, 1] = np.inf
            uv[0, 0, 1, 0] = -np.inf
            uv_da[0, 1, 0, 2] = np.nan            # a NaN differential: lod 0
    elif kind == 'boundary':
        j = np.arange(B * H * W).reshape(B, H, W)
        uv = np.stack([((7 * j) % (6 * TW) - 2 * TW) / (2.0 * TW), ((5 * j + 3) % (6 * TH) - 2 * TH) / (2.0 * TH)], -1).astype(f32)
        uv_da = np.zeros((B, H, W, 4), f32)
        k = j % (Lmax + 3)                          # lod = k exactly: 0 .. Lmax + 2
        uv_da[..., 0] = (2.0 ** k) / TW
        uv_da[j % 2 == 1, 0] = 0
        uv_da[j % 2 == 1, 3] = ((2.0 ** k) / TH)[j % 2 == 1]
    elif kind == 'runs':
        assert sum(RUN_LENGTHS) == B * H * W
        texel = np.repeat(np.arange(len(RUN_LENGTHS)) * 3 + 1, RUN_LENGTHS)           # five of the sixteen texels
        rng.shuffle(texel)
        ty, tx = texel // TW, texel % TW
        uv = np.stack([(tx + 0.5) / TW, (ty + 0.5) / TH], -1).reshape(B, H, W, 2).astype(f32)
        uv_da = np.zeros((B, H, W, 4), f32)
    else:                                           # magnify
        iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        uv = np.stack([(ix + 0.5) / W, (iy + 0.5) / H], -1)[None].repeat(B, 0).astype(f32)
        uv_da = np.zeros((B, H, W, 4), f32)
        uv_da[..., 0], uv_da[..., 3] = 1.0 / W, 1.0 / H
    return _freeze(dict(tex=tex, uv=uv, uv_da=uv_da, dout=dout, TH=TH, TW=TW, C=C, Bt=Bt, B=B, H=H, W=W, kind=kind, max_mip_level=mm, Lmax=Lmax))


@functools.lru_cache(None)
def reference(name, filt, boundary):
    """one case in one mode, read-only: px32 / px64 / pxplain (kernel float32, float64 with true log2, float32 with numpy's log2), out*, duv*,
    dtex* (32: kernel order; 64: closed form in float64; plain: float32 with no named order), `undecided` (B,H,W), `keep_texels` (Bt,TH,TW), `runs`"""
    c = case(name)
    args = (c['uv'], c['uv_da'], c['TH'], c['TW'], filt, boundary, c['max_mip_level'])
    mm = c['max_mip_level']
    px32, px64, pxp = pixel(*args, np.float32, 'poly'), pixel(*args, np.float64, 'numpy'), pixel(*args, np.float32, 'numpy')
    out = dict(px32=px32, px64=px64, pxplain=pxp, undecided=undecided(px32, px64) | undecided(pxp, px64), runs=run_lengths(px32))
    for tag, px, dt in (('32', px32, np.float32), ('64', px64, np.float64), ('plain', pxp, np.float32)):
        out['out' + tag] = forward(c['tex'], px, mm, dt)
        out['duv' + tag] = duv_closed(c['tex'], px, c['dout'], mm, dt)
    out['dtex32'] = dtex_kernel_order(px32, c['dout'], c['Bt'])
    out['dtex64'] = dtex_closed(px64, c['dout'], c['Bt'], np.float64)
    out['dtexplain'] = dtex_closed(pxp, c['dout'], c['Bt'], np.float32)
    # the texels no undecided pixel reaches, through any level, in any of the three evaluations (the weights are >= 0: nothing cancels)
    mark = out['undecided'][..., None].astype(np.float64)
    out['keep_texels'] = ~np.any([dtex_closed(px, mark, c['Bt'], np.float64)[..., 0] != 0 for px in (px32, px64, pxp)], axis=0)
    return _freeze(out)


@functools.lru_cache(None)
def sphere_scene(H, W, views=2):
    """the sphere of raster_ref with per-vertex uv (longitude, latitude) and a (V,2) second attribute set: pos, faces, r32, r64, uv_vert"""
    ref = R.sphere_reference(H, W, views)
    v, _ = R.uv_sphere()
    lon = np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5
    lat = np.arccos(np.clip(v[:, 1] / 0.5, -1, 1)) / np.pi
    return _freeze(dict(pos=ref['pos'], faces=ref['faces'], r32=ref['r32'], r64=ref['r64'], uv_vert=np.stack([lon, lat], -1).astype(f32)))


# ---- render_textured by value and the end-to-end fit ----------------------------------------------------------------------------------
@functools.lru_cache(None)
def render_reference(H, W, R_S, TS=16, C=3):
    """the texture-only branch of render_textured on two views of the sphere, rasterised at R_S (H, W): pos (the clip-space positions, which
    the test feeds through an identity K), faces, uv_vert, img (1,TS,TS,C, top row first), and the [rgb, mask] maps BEFORE the resize as
    `full64` (the float64 pipeline) and `full32` (a plain float32 one: plain32's barycentrics, numpy's log2), `decided` (B,RH,RW): the
    source pixels on which the kernel-order float32 pipeline and the float64 one hold the same face, the same texel cells and level"""
    RH, RW = H * R_S, W * R_S
    s = sphere_scene(RH, RW, 2)
    pos, faces, uvv = s['pos'], s['faces'], s['uv_vert']
    img = np.random.default_rng(R._seed(f'render {TS} {C}')).uniform(0, 1, (1, TS, TS, C)).astype(f32)
    tex = img[:, ::-1].copy()
    full, pxs = {}, {}
    for tag, dt, log2, rast in (('64', np.float64, 'numpy', s['r64']), ('32', np.float32, 'numpy', dict(s['r32'], uv=R.plain32(pos, faces, s['r32']['face'], RH, RW)['uv'])),
                                ('kernel', np.float32, 'poly', s['r32'])):
        face = rast['face']
        puv = R.interp(uvv, faces, rast['uv'], face, dt)
        da = attr_da(uvv, faces, face, rast_db(pos, faces, face, RH, RW, dt), [0, 1], dt)
        px = pixel(puv, da, TS, TS, TRILINEAR, 'wrap', 8, dt, log2)
        rgb = np.where((face >= 0)[..., None], forward(tex, px, 8, dt), 0)
        full[tag], pxs[tag] = np.concatenate([rgb, (face >= 0)[..., None].astype(dt)], -1), px
    decided = s['r64']['decided'] & (s['r64']['face'] == s['r32']['face']) & ~undecided(pxs['kernel'], pxs['64'])
    return _freeze(dict(pos=pos, faces=faces, uv_vert=uvv, img=img, full64=full['64'], full32=full['32'], full_kernel=full['kernel'], decided=decided))


FIT_STEPS, FIT_LR = 40, 0.01         # a step of 0.04 diverges in float64; 0.01 leaves a factor of four


@functools.lru_cache(None)
def fit_inputs(H=64, W=64, TS=16, C=3):
    """the end-to-end fit: uv and uv_da of two views of the sphere in the float32 kernel order (the device's bits), the texture to recover"""
    s = sphere_scene(H, W, 2)
    face = s['r32']['face']
    uv = R.interp(s['uv_vert'], s['faces'], s['r32']['uv'], face, f32)
    da = attr_da(s['uv_vert'], s['faces'], face, rast_db(s['pos'], s['faces'], face, H, W, f32), [0, 1], f32)
    true = np.random.default_rng(R._seed(f'fit {TS} {C}')).uniform(0, 1, (1, TS, TS, C)).astype(f32)
    return _freeze(dict(uv=uv, uv_da=da, mask=face >= 0, tex=true))


def fit_float64(steps=FIT_STEPS, lr=FIT_LR):
    """the fit's loop in float64 torch on the CPU: plain gradient descent on sum((texture(t) - texture(true))^2 over the covered pixels) from
    t = 0.5 -> the losses before each step and after the last"""
    import torch
    fi = fit_inputs()
    px = pixel(fi['uv'], fi['uv_da'], fi['tex'].shape[1], fi['tex'].shape[2], TRILINEAR, 'wrap', 8, np.float64, 'numpy')
    uv = torch.tensor(fi['uv'], dtype=torch.float64)
    mask = torch.tensor(fi['mask'].copy())[..., None]
    target = texture_torch(torch.tensor(fi['tex'], dtype=torch.float64), uv, px, 8)
    t = torch.full(fi['tex'].shape, 0.5, dtype=torch.float64, requires_grad=True)
    losses = []
    for _ in range(steps + 1):
        loss = (((texture_torch(t, uv, px, 8) - target) * mask) ** 2).sum()
        losses.append(float(loss.detach()))
        g, = torch.autograd.grad(loss, t)
        with torch.no_grad():
            t -= lr * g
    return losses

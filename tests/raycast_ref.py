"""References of the ray-casting tests, in numpy, and the meshes and rays they share.

    moller_trumbore(o, d, tris, dtype)      the reference's formula (lib/utils/mesh_utils.py:710-738) with its eps, in its order of
                                            operations, for every (ray, triangle) pair.  In float64 it is the truth of the tests; in
                                            float32 it is what the reference computes.
    kernel32(o, d, tris)                    the float32 restatement of the kernel's named operations (csrc/ra_raycast_tri.hpp:
                                            raycast_tri): u, v, t, det.  Its own error against the truth sets the tolerance of the
                                            parity tests (the 10 x float32 rule) and the classification margin below.
    accept_ref(u, v, t)                     the reference's predicate
    accept_kernel32(o, d, tris, u, v, t, det)   the kernel's: the reference's, the grazing guard and the slab clause (raycast_hit)
    nearest_count(accept, u, v, t)          exhaustive nearest hit (lowest t, then lowest face index) and count on top of either

THE CLASSIFICATION CONDITION (stated once, here).  A pair is DECIDED when, in the float64 restatement,
    min(|u|, |v|, |1 - u - v|, |t|) > margin   and   |det| / (|d| |N|) > margin;
a ray is decided when all its pairs are.  The margin of a (mesh, ray set) is 10 x the largest error of kernel32 against float64 —
max(|du|, |dv|, |dt| / max(1, |t|)) — over that set's well-conditioned hits, the pairs float64 accepts with |det| / (|d| |N|) >=
WELL (the project's 10 x float32 rule; a hit at a grazing angle has an error that grows with 1 / cos and says nothing about the
arithmetic).  On a decided ray no comparison of the predicate is within the margin of flipping, so face and count of the float64
exhaustive result are what any correct float32 evaluation must return.  A face of exactly no area has |N| = 0 and decides nothing: on
the mesh 'degenerate' no ray is decided, and only bit-equality, determinism and finiteness are asserted there, as on the ray set GRAZE.
"""
import functools

import numpy as np

import winding_ref as W

MESHES = ('hull', 'two', 'far', 'degenerate', 'flipped', 'single')
SETS = ('outside', 'inside', 'miss', 'km')          # the non-degenerate ray sets
GRAZE = 'graze'                                     # coplanar, parallel, edge, vertex, d = 0: a separate set
SIZES = {'outside': 257, 'inside': 130, 'miss': 130, 'km': 4, 'graze': 130}
WELL = 0.1
UNDECIDED_CAP = 0.02
EPS = 1e-8
F32 = np.float32
BOX_PAD, DET_ROUND, GUARD, SLAB_REL = F32(2.0 ** -19), F32(2.0 ** -21), F32(1), F32(2.0 ** -6)       # ra_mesh_tri.hpp, ra_raycast_tri.hpp
GOLDEN_MESHES = ('hull', 'far')
GOLDEN_FACE_STEP = 10


def mesh_case(name):
    return W.mesh_case(name)


def tris_of(name, dtype=np.float64):
    v, f = mesh_case(name)
    return v.astype(dtype)[f]


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(None)
def ray_sets(name):
    """{set: (o, d)} float32.  outside: from 0.3 .. 3 m outside towards interior points of faces (barycentrics >= 0.1), d of any
    length; inside: from inside the first hull outwards; miss: from outside the mesh's bounding sphere, pointing away; km: origins
    1 km away aimed at interior points; graze: in a face's plane, parallel 1 mm above it, through shared-edge midpoints, through
    vertices, d = 0."""
    v, f = mesh_case(name)
    v64 = v.astype(np.float64)
    tri = v64[f]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    good = np.nonzero(np.linalg.norm(nrm, axis=-1) > 1e-8)[0]          # faces with a normal
    rng = np.random.default_rng(20)
    hv = W.hull()[0].astype(np.float64)
    cen_a = hv.mean(0) + (W.FAR_OFFSET if name == 'far' else 0)       # the centre of the first hull
    cen_all, radius = v64.mean(0), 2 * np.linalg.norm(v64 - v64.mean(0), axis=-1).max()

    def aimed(n, dist_lo, dist_hi, jitter):
        idx = good[rng.integers(0, len(good), n)]
        b = 0.1 + 0.7 * rng.dirichlet([1, 1, 1], n)
        target = (b[:, :, None] * tri[idx]).sum(1)
        un = _unit(nrm[idx])
        side = np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None] if name == 'single' else np.sign(((target - np.where(target[:, :1] > cen_a[0] + 2.5, cen_a + [5, 0, 0], cen_a)) * un).sum(-1, keepdims=True))
        dist = rng.uniform(dist_lo, dist_hi, (n, 1))
        o = target + dist * (side * un + jitter * rng.normal(size=(n, 3)))
        return o, (target - o) * rng.uniform(0.2, 5.0, (n, 1)), idx, target

    sets = {}
    o, d, _, _ = aimed(SIZES['outside'], 0.3, 3.0, 0.3)
    sets['outside'] = (o, d)
    n = SIZES['inside']
    o = cen_a + 0.3 * (hv[rng.integers(0, len(hv), n)] + (W.FAR_OFFSET if name == 'far' else 0) - cen_a)
    sets['inside'] = (o, rng.normal(size=(n, 3)) * rng.uniform(0.2, 5.0, (n, 1)))
    n = SIZES['miss']
    out = _unit(rng.normal(size=(n, 3)))
    sets['miss'] = (cen_all + radius * out, (out + 0.3 * rng.normal(size=(n, 3))) * rng.uniform(0.2, 5.0, (n, 1)))
    o, d, _, _ = aimed(SIZES['km'], 1000.0, 1000.0, 0.05)
    sets['km'] = (o, d)
    # the degenerate set
    k = 26
    idx = good[rng.integers(0, len(good), k)]
    a, c = tri[idx, 0], tri[idx].mean(1)
    un = _unit(nrm[idx])
    o1 = c + 3.0 * (a - c)                                           # in the plane, outside the face, aimed through it
    go, gd = [o1, o1 + 1e-3 * un], [c - o1, c - o1]                    # ... and the same direction 1 mm above the plane
    mid = 0.5 * (tri[idx, 0] + tri[idx, 1])                          # a shared edge's midpoint
    for target in (mid, a):                                          # ... and a vertex
        o = target + rng.uniform(0.5, 2.0, (k, 1)) * (un + 0.3 * rng.normal(size=(k, 3)))
        go.append(o), gd.append(target - o)
    go.append(sets['outside'][0][:k]), gd.append(np.zeros((k, 3)))   # d = 0
    sets[GRAZE] = (np.concatenate(go), np.concatenate(gd))
    sets = {s: (np.ascontiguousarray(o.astype(F32)), np.ascontiguousarray(d.astype(F32))) for s, (o, d) in sets.items()}
    assert all(len(sets[s][0]) == SIZES[s] for s in sets), {s: len(sets[s][0]) for s in sets}
    return sets


def checksum(name, group):
    v, f = mesh_case(name)
    o, d = ray_sets(name)[group]
    return np.array([v.astype(np.float64).sum(), float(f.sum()), o.astype(np.float64).sum(), d.astype(np.float64).sum(), len(f), len(o)])


def golden_pairs(name):
    """the small pair set of the golden: 48 + 16 + 16 + 4 rays of the four sets against every 10th face"""
    s = ray_sets(name)
    o = np.concatenate([s['outside'][0][:48], s['inside'][0][:16], s['miss'][0][:16], s['km'][0]])
    d = np.concatenate([s['outside'][1][:48], s['inside'][1][:16], s['miss'][1][:16], s['km'][1]])
    return o, d, tris_of(name, F32)[::GOLDEN_FACE_STEP]


# ------------------------------------------------------------------------------------------------ the reference's formula
def moller_trumbore(o, d, tris, dtype=np.float64):
    """(n, 3), (n, 3), (F, 3, 3) -> u, v, t, det of shape (n, F) in dtype: the reference's operations in its order (torch sums three
    products left to right)"""
    o, d, tris = (np.asarray(x, dtype=dtype) for x in (o, d, tris))
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(e1, e2)

    def dot(a, b):
        p = a * b
        return (p[..., 0] + p[..., 1]) + p[..., 2]
    with np.errstate(all='ignore'):
        det = dot(d[:, None, :], n[None])
        invdet = dtype(1) / -(det + dtype(EPS))
        a0 = o[:, None, :] - tris[None, :, 0]
        da0 = np.cross(a0, np.broadcast_to(d[:, None, :], a0.shape))
        u = dot(da0, e2[None]) * invdet
        v = -dot(da0, e1[None]) * invdet
        t = dot(a0, n[None]) * invdet
    assert u.dtype == dtype
    return u, v, t, det


def accept_ref(u, v, t):
    with np.errstate(invalid='ignore'):
        return (t >= 0) & (u >= 0) & (v >= 0) & (u + v <= 1)


# ------------------------------------------------------------------------------------------------ the kernel's operations, in float32
_fma32, _dot32 = W._fma32, W._dot32


def _cross32(a, b):
    return np.stack([_fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     _fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)


def kernel32(o, d, tris):
    """raycast_tri on float32 arrays: u, v, t, det of shape (n, F), float32"""
    o, d, tris = (np.asarray(x, dtype=F32) for x in (o, d, tris))
    a = tris[None, :, 0]
    e1, e2 = tris[None, :, 1] - a, tris[None, :, 2] - a
    n = _cross32(e1, e2)
    dd = np.broadcast_to(d[:, None, :], (len(o), tris.shape[0], 3))
    with np.errstate(all='ignore'):
        det = _dot32(dd, np.broadcast_to(n, dd.shape))
        invdet = F32(1) / -(det + F32(EPS))
        a0 = o[:, None, :] - a
        da0 = _cross32(a0, dd)
        u = _dot32(da0, np.broadcast_to(e2, dd.shape)) * invdet
        v = -_dot32(da0, np.broadcast_to(e1, dd.shape)) * invdet
        t = _dot32(a0, np.broadcast_to(n, dd.shape)) * invdet
    assert u.dtype == v.dtype == t.dtype == det.dtype == F32
    return u, v, t, det


def face_box32(tris):
    """ray_face_box: (F, 6)"""
    tris = np.asarray(tris, dtype=F32)
    lo, hi = tris.min(1), tris.max(1)
    pad = (np.maximum(np.abs(lo), np.abs(hi)).max(-1) * BOX_PAD)[:, None]
    return np.concatenate([lo - pad, hi + pad], -1).astype(F32)


def slab32(o, d, box):
    """ray_slab of rays (n, 3) against boxes (F, 6): lo_t, hi_t of shape (n, F), float32"""
    o, d, box = (np.asarray(x, dtype=F32) for x in (o, d, box))
    with np.errstate(all='ignore'):
        inv = (F32(1) / d)[:, None, :]
        flat = ~(np.abs(inv) < np.inf)
        inv = np.copysign(np.maximum(np.abs(inv), F32(2.0 ** -126)), inv)          # RAY_INV_MIN
        lo, hi, oo = box[None, :, :3], box[None, :, 3:], o[:, None, :]
        t1, t2 = (lo - oo) * inv, (hi - oo) * inv
        inside = (lo <= oo) & (oo <= hi)
        near = np.where(flat, np.where(inside, -np.inf, np.inf), np.fmin(t1, t2)).astype(F32)
        far = np.where(flat, np.where(inside, np.inf, -np.inf), np.fmax(t1, t2)).astype(F32)
        entry, leave = near.max(-1), far.min(-1)
        some = (box[:, 0] <= box[:, 3])[None]
        lo_t = np.where(some, _fma32(-SLAB_REL, np.abs(entry), entry), F32(np.inf))
        hi_t = np.where(some, _fma32(SLAB_REL, np.abs(leave), leave), F32(-np.inf))
    return lo_t.astype(F32), hi_t.astype(F32)


def guard32(d, tris, det):
    d, tris = np.asarray(d, dtype=F32), np.asarray(tris, dtype=F32)
    e1, e2 = np.abs(tris[:, 1] - tris[:, 0]), np.abs(tris[:, 2] - tris[:, 0])
    nabs = np.stack([_fma32(e1[:, 1], e2[:, 2], e1[:, 2] * e2[:, 1]), _fma32(e1[:, 2], e2[:, 0], e1[:, 0] * e2[:, 2]),
                     _fma32(e1[:, 0], e2[:, 1], e1[:, 1] * e2[:, 0])], -1)
    shape = (len(d), len(tris), 3)
    s = _dot32(np.broadcast_to(np.abs(d)[:, None, :], shape), np.broadcast_to(nabs[None], shape))
    return np.abs(det) > (GUARD * DET_ROUND) * s


def accept_kernel32(o, d, tris, u, v, t, det):
    lo_t, hi_t = slab32(o, d, face_box32(tris))
    with np.errstate(invalid='ignore'):
        return accept_ref(u, v, t) & guard32(d, tris, det) & (lo_t <= t) & (t <= hi_t)


def nearest_count(accept, u, v, t):
    """t (+inf), face (-1), uv (NaN), count per ray: the lowest t, then the lowest face index"""
    if accept.shape[1] == 0:                     # a mesh without a kept face
        n = len(accept)
        return np.full(n, np.inf, t.dtype), np.full(n, -1, np.int32), np.full((n, 2), np.nan, t.dtype), np.zeros(n, np.int32)
    tt = np.where(accept, t, np.inf)
    face = tt.argmin(1)                          # the first index of the minimum
    rows = np.arange(len(tt))
    hit = accept.any(1)
    best = tt[rows, face]
    uv = np.stack([u[rows, face], v[rows, face]], -1)
    uv[~hit] = np.nan
    return best, np.where(hit, face, -1).astype(np.int32), uv, accept.sum(1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ classification
def evaluate_mesh(o, d, verts, faces):
    """everything the tests need of rays against a mesh: float64 truth, the reference in float32, the kernel's restatement, the margin,
    the decided rays.  A face with a non-finite vertex is dropped, as ra_mesh_create drops it; face indices are the caller's."""
    o, d = np.asarray(o, dtype=F32), np.asarray(d, dtype=F32)
    tri = np.asarray(verts, dtype=F32)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    kept = np.nonzero(np.isfinite(tri).all((1, 2)))[0]
    tri32, tri64 = tri[kept], tri[kept].astype(np.float64)
    u64, v64, t64, det64 = moller_trumbore(o, d, tri64, np.float64)
    u32, v32, t32, _ = moller_trumbore(o, d, tri32, F32)
    uk, vk, tk, detk = kernel32(o, d, tri32)
    acc64, acc32, acck = accept_ref(u64, v64, t64), accept_ref(u32, v32, t32), accept_kernel32(o, d, tri32, uk, vk, tk, detk)
    n64 = np.cross(tri64[:, 1] - tri64[:, 0], tri64[:, 2] - tri64[:, 0])
    with np.errstate(all='ignore'):
        cosang = np.abs(det64) / (np.linalg.norm(d.astype(np.float64), axis=-1)[:, None] * np.linalg.norm(n64, axis=-1)[None])
        err = np.maximum(np.maximum(np.abs(uk - u64), np.abs(vk - v64)), np.abs(tk - t64) / np.maximum(1, np.abs(t64)))
        well = acc64 & (cosang >= WELL)
        measured = float(err[well].max()) if well.any() else 2.0 ** -23
        margin = 10 * measured
        pair_decided = (np.minimum(np.minimum(np.abs(u64), np.abs(v64)), np.minimum(np.abs(1 - u64 - v64), np.abs(t64))) > margin) & (cosang > margin)

    def original(res):
        t, face, uv, count = res
        return t, np.where(face >= 0, kept[np.maximum(face, 0)] if len(kept) else -1, -1).astype(np.int32), uv, count
    return dict(o=o, d=d, u64=u64, v64=v64, t64=t64, acc64=acc64, acc32=acc32, acck=acck, uk=uk, vk=vk, tk=tk, u32=u32, v32=v32, t32=t32,
                margin=margin, measured=measured, pair_decided=pair_decided, decided=pair_decided.all(1),
                truth=original(nearest_count(acc64, u64, v64, t64)), restated=original(nearest_count(acck, uk, vk, tk)))


@functools.lru_cache(None)
def evaluate(name, group):
    """evaluate_mesh of a (mesh, ray set), computed once"""
    return evaluate_mesh(*ray_sets(name)[group], *mesh_case(name))


NEAR = 2.0          # a pair is NEAR its face when float64 |u| and |v| are at most this: the ray meets the face's plane within one edge length of it


def near_pairs(u64, v64):
    with np.errstate(invalid='ignore'):
        return (np.abs(u64) <= NEAR) & (np.abs(v64) <= NEAR)


def check_pairs(tag, got, g32, g64, near):
    """dense u, v or t against the golden.
      - the 10 x rule (frame_stage_ref.parity) on maximum and median of all pairs, normalised by the largest value and per element;
      - the ceiling "no worse than the reference in float32" on the MEDIAN of all pairs;
      - the ceiling on the MAXIMUM over the pairs NEAR their face (near: the mask of near_pairs; every pair float64 accepts is one),
        the pairs whose u, v, t can decide a hit: max |got - float64| <= max |reference float32 - float64| + one float32 ulp of the
        largest value there (2^-23 max(1, |value|)).  The allowance is the final rounding: the kernel evaluates the reference's own
        formula, so on its worst pair it can end one rounding of the result away from the reference's float32 on either side.
        Over ALL pairs the maximum sits on one ray that is parallel to a face to rounding (|u| about 2e4), where either arithmetic's
        error is its rounding of det times 1 / det^2: measured ratios 0.28 (hull) and 1.74 (far); that pair is under the 10 x rule."""
    from frame_stage_ref import parity
    parity(tag, got, g32, g64)
    parity(f'{tag}, per element', got, g32, g64, relative=True)
    ek, e32 = np.abs(np.asarray(got, dtype=np.float64) - g64), np.abs(g32.astype(np.float64) - g64)
    scale = np.maximum(1, np.abs(g64))
    e, own = np.median(ek / scale), np.median(e32 / scale)
    print(f'{tag}: median |. - float64| {e:.3e}, the reference in float32 {own:.3e}, ratio {e / own:.3f}')
    assert e <= own, tag
    assert near.sum() >= 100, tag
    ulp = 2.0 ** -23 * scale[near].max()
    e, own = ek[near].max(), e32[near].max()
    print(f'{tag}: {int(near.sum())} pairs near their face: max |. - float64| {e:.3e}, the reference in float32 {own:.3e}, ratio {e / own:.3f}; '
          f'above it by {(e - own) / ulp:.2f} of the allowed ulp {ulp:.3e}')
    assert e <= own + ulp, tag

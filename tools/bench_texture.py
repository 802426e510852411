"""The texture path: time per call (HIP events, warm clocks, one process).  One JSON line:

    camera320k   bench_rasterize's scene — 512 x 512 pixels, a pinhole 3 m in front of the 320 000-face mesh — with per-vertex texture
                 coordinates (longitude, height) and a 1024 x 1024 x 3 texture

Legs, the legs interleaved:
    differentials     Engine.raster_db, then Engine.interpolate_da of the two uv channels
    texture_nearest, texture_linear, texture_trilinear     Engine.texture in each filter mode (boundary wrap, max_mip_level 8; the trilinear
                      leg builds the mip chain inside the call)
    backward          Engine.texture_backward (duv and dtex) of the trilinear forward; backward_duv alone, and sort_share = 1 - the time
                      of the same call without dtex, so an UPPER bound on the sort's share (keys, sort, runs and fold together)
    backward_covered  the same backward with a NaN uv on the empty pixels, as render_textured passes them: a NaN uv emits no tap, whereas
                      Engine.interpolate's uv = (0, 0) sends every empty pixel's four taps to the same four texels — four runs of
                      (empty pixels) taps, each summed by ONE wave
    raster            Engine.rasterize, then Engine.interpolate of 3 channels, of the same frame in the same run

    python tools/bench_texture.py [--out profiles/texture.jsonl] [--reps 10]

CONDITION: the trilinear forward's median is not above the median of `raster` in the same run (no margin: a per-pixel eight-tap gather
that costs more than binning and drawing 320 000 faces points to a mistake).  The line says whether it holds; the tool exits 1 when it
does not.  The backward has no bar.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_mesh_distance import SCALE, stats, subdivide, template, timed
from bench_rasterize import DIST, FOV
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'texture.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--image', type=int, default=512)
    ap.add_argument('--texture', type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    dev = eng.device
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    v = v * SCALE
    H, TS = args.image, args.texture
    tv = torch.from_numpy(v.astype(np.float32)).to(dev)
    tf = torch.from_numpy(f.astype(np.int32)).to(dev)
    s = DIST / FOV
    pos = torch.stack([tv[:, 0] * s, -tv[:, 2] * s, torch.full_like(tv[:, 0], -0.02), tv[:, 1] + DIST], -1)[None].contiguous()
    lon = torch.atan2(tv[:, 1], tv[:, 0]) / (2 * np.pi) + 0.5
    height = (tv[:, 2] - tv[:, 2].min()) / (tv[:, 2].max() - tv[:, 2].min())
    uv_vert = torch.stack([lon, height], -1).contiguous()
    attrs = torch.rand(tv.shape[0], 3, device=dev)
    tex = torch.rand(1, TS, TS, 3, device=dev)
    rast = eng.rasterize(pos, tf, H, H)
    rast_db = eng.raster_db(pos, tf, rast)
    uv = eng.interpolate(uv_vert, rast, tf)
    uv_da = eng.interpolate_da(uv_vert, rast, tf, rast_db, [0, 1])
    dout = torch.rand(1, H, H, 3, device=dev)
    uv_nan = torch.where((rast.face >= 0)[..., None], uv, torch.full_like(uv, float('nan'))).contiguous()
    legs = {'raster': lambda: eng.interpolate(attrs, eng.rasterize(pos, tf, H, H), tf),
            'differentials': lambda: eng.interpolate_da(uv_vert, rast, tf, eng.raster_db(pos, tf, rast), [0, 1]),
            'texture_nearest': lambda: eng.texture(tex, uv, None, 'nearest'),
            'texture_linear': lambda: eng.texture(tex, uv, None, 'linear'),
            'texture_trilinear': lambda: eng.texture(tex, uv, uv_da, 'linear-mipmap-linear', 'wrap', 8),
            'backward': lambda: eng.texture_backward(tex, uv, dout, uv_da, 'linear-mipmap-linear', 'wrap', 8),
            'backward_covered': lambda: eng.texture_backward(tex, uv_nan, dout, uv_da, 'linear-mipmap-linear', 'wrap', 8),
            'backward_duv': lambda: eng.texture_backward(tex, uv, dout, uv_da, 'linear-mipmap-linear', 'wrap', 8, want=('duv',))}
    for fn in legs.values():         # warm-up of every leg
        fn()
    torch.cuda.synchronize()
    lod = 0.5 * torch.log2(((uv_da[..., 0] * TS) ** 2 + (uv_da[..., 1] * TS) ** 2 + (uv_da[..., 2] * TS) ** 2 + (uv_da[..., 3] * TS) ** 2).clamp_min(1e-30))
    covered = rast.face >= 0
    line = dict(tool='bench_texture', shape='camera320k', note=f'{H} x {H} pixels from 3 m, {len(f)} faces, texture {TS} x {TS} x 3, max_mip_level 8',
                faces=int(len(f)), verts=int(len(v)), image=[H, H], texture=[TS, TS, 3], reps=args.reps, device=torch.cuda.get_device_name(0),
                covered_share=float(covered.float().mean()), median_lod_upper_estimate=float(lod[covered].median()))
    t = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    for k in t:
        stats(line, k, t[k])
    line['sort_share_upper_bound'] = round(1.0 - line['backward_duv_ms'] / line['backward_ms'], 3)
    line['sort_share_upper_bound_covered'] = round(1.0 - line['backward_duv_ms'] / line['backward_covered_ms'], 3)
    line['trilinear_over_raster'] = round(line['texture_trilinear_ms'] / line['raster_ms'], 3)
    line['condition_trilinear_not_above_raster'] = bool(line['texture_trilinear_ms'] <= line['raster_ms'])
    s = json.dumps(line)
    print(s)
    with open(args.out, 'w') as fh:
        fh.write(s + '\n')
    return 0 if line['condition_trilinear_not_above_raster'] else 1


if __name__ == '__main__':
    sys.exit(main())

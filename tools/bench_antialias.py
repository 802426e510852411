"""ra_antialias and its two backward passes beside ra_rasterize + ra_interpolate of the same frame: time per call (HIP events, warm
clocks, one process).  One JSON line per shape, bench_rasterize's camera and meshes:

    camera320k   512 x 512 pixels, a pinhole 3 m in front of a mesh of 320 000 faces
    body13776    the same camera on the 13 776-face hull of the 6 890-vertex template

Legs, 4 channels:
    raster         Engine.rasterize, then Engine.interpolate — what the antialiasing op is added to
    antialias      Engine.antialias on that frame's maps
    dcolor, dpos   Engine.antialias_backward with want=('dcolor',) and want=('dpos',)
    backward       both in one call

    python tools/bench_antialias.py [--out profiles/antialias.jsonl] [--reps 10]

Every leg is warmed up (code objects, ctx scratch, clocks), then timed `reps` times, the legs interleaved; the median and min .. max
are reported.  No target is fixed here: the numbers are written down (DESIGN.md section 26 compares antialias with raster).
A run without a HIP device fails: there is no CPU fallback.
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

CHANNELS = 4


def run_shape(eng, name, verts, faces, H, reps, note):
    dev = eng.device
    tv = torch.from_numpy(verts.astype(np.float32)).to(dev)
    tf = torch.from_numpy(faces.astype(np.int32)).to(dev)
    s = DIST / FOV
    pos = torch.stack([tv[:, 0] * s, -tv[:, 2] * s, torch.full_like(tv[:, 0], -0.02), tv[:, 1] + DIST], -1)[None].contiguous()
    attrs = torch.rand(tv.shape[0], CHANNELS, device=dev)
    topo = eng.topology(tf, tv.shape[0])
    rast = eng.rasterize(pos, tf, H, H)
    color = eng.interpolate(attrs, rast, tf)
    dout = torch.rand(1, H, H, CHANNELS, device=dev)
    legs = {'raster': lambda: eng.interpolate(attrs, eng.rasterize(pos, tf, H, H), tf), 'antialias': lambda: eng.antialias(topo, color, rast, pos),
            'dcolor': lambda: eng.antialias_backward(topo, color, rast, pos, dout, want=('dcolor',)),
            'dpos': lambda: eng.antialias_backward(topo, color, rast, pos, dout, want=('dpos',)),
            'backward': lambda: eng.antialias_backward(topo, color, rast, pos, dout)}
    for fn in legs.values():         # warm-up of every leg
        fn()
    torch.cuda.synchronize()
    out = eng.antialias(topo, color, rast, pos)
    f = rast.face[0]
    differ = int((f[:, 1:] != f[:, :-1]).sum()) + int((f[1:] != f[:-1]).sum())
    line = dict(tool='bench_antialias', shape=name, note=note, faces=int(len(faces)), verts=int(len(verts)), image=[H, H], channels=CHANNELS, reps=reps,
                device=torch.cuda.get_device_name(0), covered_share=float((f >= 0).float().mean()), pairs_with_two_faces=differ,
                pixels_changed=int((out != color).any(-1).sum()))
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    for k in t:
        stats(line, k, t[k])
    line['antialias_over_raster'] = round(line['antialias_ms'] / line['raster_ms'], 3)
    topo.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'antialias.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--image', type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    lines = []
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    lines.append(run_shape(eng, 'camera320k', v * SCALE, f, args.image, args.reps, f'{args.image} x {args.image} pixels from 3 m, {len(f)} faces'))
    v, f = template(6890)
    lines.append(run_shape(eng, 'body13776', v * SCALE, f, args.image, args.reps, f'{args.image} x {args.image} pixels from 3 m, {len(f)} faces'))
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

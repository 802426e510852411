"""ra_mesh_raycast at the two shapes the project has a use for: time per call (HIP events, warm clocks, one process).
One JSON line per shape:

    camera    512 x 512 pinhole rays from 3 m, nearest hit (t, face, uv: pruned by t), against a mesh of 320 000 faces (the synthetic
              template at 2 502 vertices, subdivided three times onto its ellipsoid): an extracted mesh seen from a dataset camera
    stabbing  1 000 000 points within 0.1 m of a 13 776-face body (the 6 890-vertex template's hull: SMPL's counts), one ray each in
              the direction ray_stabbing draws (normalize(rand)), count mode: nothing is pruned by t

Per shape four legs: the default sweep (rays Morton-sorted by origin internally), the sweep on the rays as given (RA_RAYCAST_UNSORTED),
RA_RAYCAST_BRUTE, and the reference's way — the dense ra_ray_tri_pairs and a torch reduction over its (n, F) arrays — on as many
rays as keep n x F under 2^30 (its time is also given scaled to all rays).  The three raycast legs must agree bit for bit at the timed
sizes, and the dense leg must give the same hit mask / count parity wherever no pair sits on the guard; the line says so.

    python tools/bench_mesh_raycast.py [--out profiles/mesh_raycast.jsonl] [--reps 10]

Every leg, the exhaustive and the dense one too, is warmed up (code objects, ctx scratch, clocks), then timed `reps` times, the legs
interleaved; the median and the spread are reported.  No target is fixed: the numbers are written down.  A run without a HIP device fails: there is no CPU fallback.
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
from relightableavatar_amd import mesh_utils
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def dense(eng, o, d, tris, count):
    """the reference's moller_trumbore and the reduction ray_stabbing / a nearest-hit search makes over it"""
    u, v, t = eng.ray_tri_pairs(o, d, tris)
    hit = (t >= 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    if count:
        return hit.count_nonzero(dim=-1)
    return torch.where(hit, t, torch.full((), float('inf'), device=t.device)).min(dim=-1)[0]


def run_shape(eng, name, verts, faces, o, d, want, reps, note):
    dev = eng.device
    tv, tf = torch.from_numpy(verts.astype(np.float32)).to(dev), torch.from_numpy(faces.astype(np.int32))
    o, d = o.to(dev).float().contiguous(), d.to(dev).float().contiguous()
    mesh = eng.mesh(tv, tf)
    legs = {'sweep': dict(), 'sweep_unsorted': dict(sort=False), 'brute': dict(brute=True)}
    outs = {k: mesh.raycast(o, d, want=want, **kw) for k, kw in legs.items()}             # warm-up of every leg, and the answers to compare
    n_dense = int(min(o.shape[0], (2 ** 30 - 1) // len(faces)))
    tris = tv[tf.to(dev).long()]
    count = 'count' in want
    dn = dense(eng, o[:n_dense], d[:n_dense], tris, count)
    torch.cuda.synchronize()
    same = all(torch.equal(outs['sweep'][k].view(torch.int32), outs[x][k].view(torch.int32)) for x in ('sweep_unsorted', 'brute') for k in want)
    if count:
        differ = int((dn != outs['sweep'].count[:n_dense]).sum())
    else:
        differ = int((torch.isfinite(dn) != (outs['sweep'].face[:n_dense] >= 0)).sum())
    del dn
    t = {k: [] for k in list(legs) + ['dense']}
    for r in range(reps):
        for k, kw in legs.items():
            t[k].append(timed(lambda: mesh.raycast(o, d, want=want, **kw)))
        t['dense'].append(timed(lambda: dense(eng, o[:n_dense], d[:n_dense], tris, count)))
    line = dict(tool='bench_mesh_raycast', shape=name, note=note, want=list(want), faces=int(len(faces)), verts=int(len(verts)), rays=int(o.shape[0]), reps=reps,
                device=torch.cuda.get_device_name(0), bit_identical=bool(same), dense_rays=n_dense, dense_differs_on=differ)
    if count:
        line['odd_share'] = float((outs['sweep'].count % 2).float().mean())
    else:
        line['hit_share'] = float((outs['sweep'].face >= 0).float().mean())
    for k in t:
        stats(line, k, t[k])
    line['dense_scaled_ms'] = round(line['dense_ms'] * o.shape[0] / n_dense, 3)
    line['brute_over_sweep'] = round(line['brute_ms'] / line['sweep_ms'], 2)
    line['unsorted_over_sweep'] = round(line['sweep_unsorted_ms'] / line['sweep_ms'], 2)
    line['pairs_per_s_brute'] = float('%.3g' % (o.shape[0] * len(faces) / (line['brute_ms'] * 1e-3)))
    mesh.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'mesh_raycast.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--image', type=int, default=512)
    ap.add_argument('--points', type=int, default=1000000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    g = torch.Generator().manual_seed(0)
    lines = []
    # a dataset camera: a pinhole 3 m in front of the body whose image just holds it
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    H = args.image
    px = (torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1
    gz, gx = torch.meshgrid(px, px, indexing='ij')
    d = torch.stack([gx * 0.55, torch.full_like(gx, 3.0), -gz * 0.55], -1).reshape(-1, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([0.0, -3.0, 0.0], dtype=torch.float64).expand_as(d)
    lines.append(run_shape(eng, 'camera', v * SCALE, f, o, d, ('t', 'face', 'uv'), args.reps, f'{H} x {H} pinhole rays from 3 m, nearest hit'))
    # ray_stabbing at SMPL's counts: points within 0.1 m of the body, the directions the reference draws
    v, f = template(6890)
    on = mesh_utils.sample_surface(torch.from_numpy(v * SCALE), torch.from_numpy(f), args.points, g)[0]
    off = torch.randn(args.points, 3, generator=g, dtype=torch.float64)
    off = off / off.norm(dim=-1, keepdim=True) * 0.1 * torch.rand(args.points, 1, generator=g, dtype=torch.float64)
    d = torch.rand(args.points, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    lines.append(run_shape(eng, 'stabbing', v * SCALE, f, on + off, d, ('count',), args.reps, 'points within 0.1 m of the surface, count mode'))
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

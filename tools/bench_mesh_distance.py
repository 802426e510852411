"""ra_mesh_create / ra_mesh_closest at the two shapes the project has a use for: time per call (HIP events, warm clocks, one process).
One JSON line per shape:

    evaluator  10 000 random samples of one surface against a mesh of 320 000 faces 3 mm away (the mesh evaluator's P2S query; the
               target is the synthetic template at 2 502 vertices, subdivided three times onto its ellipsoid)
    smpl       1 000 000 points within 0.1 m of a 13 776-face body (the 6 890-vertex template's hull: SMPL's counts), the query
               base_network.py:417-427 makes per batch of sample points

Per shape: the build (ra_mesh_create, faces already on the host), and the query three ways in the same library — the default sweep
(points Morton-sorted internally), the sweep on the points as given (RA_MESH_UNSORTED: random points share a wave), and RA_MESH_BRUTE.
The three must agree bit for bit at the timed sizes; the line says so.

    python tools/bench_mesh_distance.py [--out profiles/mesh_distance.jsonl] [--reps 10] [--brute-reps 3]

Every leg is warmed up (code objects, ctx scratch, clocks), then timed `reps` times, the legs interleaved; the median and the spread
are reported.  No target is fixed: the numbers are written down.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from relightableavatar_amd import mesh_utils, synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine

SCALE = 0.4 * np.array([0.8, 0.7, 1.1])      # synthetic.make_body's ellipsoid


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def stats(r, key, v):
    r[key + '_ms'] = round(median(v), 4)
    r[key + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def template(n_verts):
    """unit-sphere points of the synthetic template and their hull's triangles"""
    nrm = synthetic.make_body(0, posed=False, n_verts=n_verts).tverts[0].numpy().astype(np.float64) / SCALE
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return nrm, synthetic._template_faces(nrm)


def subdivide(v, f):
    """every triangle into four, the edge midpoints pushed onto the unit sphere"""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    ue, inv = np.unique(e, axis=0, return_inverse=True)
    mid = v[ue].mean(1)
    mid /= np.linalg.norm(mid, axis=-1, keepdims=True)
    m = len(v) + inv.reshape(3, -1)
    a, b, c = f.T
    return np.concatenate([v, mid]), np.concatenate([np.stack(t, 1) for t in ((a, m[0], m[2]), (m[0], b, m[1]), (m[2], m[1], c), (m[0], m[1], m[2]))])


def run_shape(eng, name, verts, faces, pts, reps, brute_reps, note):
    dev = eng.device
    tv, tf = torch.from_numpy(verts.astype(np.float32)).to(dev), torch.from_numpy(faces.astype(np.int32))
    pts = pts.to(dev).float().contiguous()
    holder = []

    def build():
        holder.append(eng.mesh(tv, tf))

    legs = {'sweep': dict(), 'sweep_unsorted': dict(sort=False), 'brute': dict(brute=True)}
    for _ in range(2):
        build()
        holder.pop().close()
    mesh = eng.mesh(tv, tf)
    outs = {k: mesh.closest(pts, **kw) for k, kw in legs.items()}             # warm-up of every leg, and the answers to compare
    torch.cuda.synchronize()
    same = all(torch.equal(outs['sweep'][k].view(torch.int32), outs[o][k].view(torch.int32)) for o in ('sweep_unsorted', 'brute') for k in outs['sweep'])
    t = {k: [] for k in list(legs) + ['build']}
    for r in range(reps):
        t['build'].append(timed(build))
        holder.pop().close()
        for k, kw in legs.items():
            if k != 'brute' or r < brute_reps:
                t[k].append(timed(lambda: mesh.closest(pts, **kw)))
    line = dict(tool='bench_mesh_distance', shape=name, note=note, faces=int(len(faces)), verts=int(len(verts)), points=int(pts.shape[0]), reps=reps,
                brute_reps=brute_reps, device=torch.cuda.get_device_name(0), bit_identical=bool(same),
                mean_distance=float(outs['sweep'].d2.double().sqrt().mean()))
    for k in t:
        stats(line, k, t[k])
    line['brute_over_sweep'] = round(line['brute_ms'] / line['sweep_ms'], 2)
    line['unsorted_over_sweep'] = round(line['sweep_unsorted_ms'] / line['sweep_ms'], 2)
    mesh.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'mesh_distance.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--brute-reps', type=int, default=3)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--smpl-points', type=int, default=1000000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    g = torch.Generator().manual_seed(0)
    lines = []
    # the evaluator's query: samples of a surface 3 mm outside the target
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    src = torch.from_numpy(v * SCALE * (1 + 0.003 / SCALE.mean()))
    pts = mesh_utils.sample_surface(src, torch.from_numpy(f), 10000, g)[0]
    lines.append(run_shape(eng, 'evaluator', v * SCALE, f, pts, args.reps, args.brute_reps, '10 000 surface samples, 3 mm from the mesh'))
    # SMPL's counts: points within 0.1 m of the body
    v, f = template(6890)
    on = mesh_utils.sample_surface(torch.from_numpy(v * SCALE), torch.from_numpy(f), args.smpl_points, g)[0]
    off = torch.randn(args.smpl_points, 3, generator=g, dtype=torch.float64)
    off = off / off.norm(dim=-1, keepdim=True) * 0.1 * torch.rand(args.smpl_points, 1, generator=g, dtype=torch.float64)
    lines.append(run_shape(eng, 'smpl', v * SCALE, f, on + off, args.reps, args.brute_reps, 'points within 0.1 m of the surface'))
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

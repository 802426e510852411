"""ra_mesh_closest_backward at bench_mesh_distance's two shapes: time per call (HIP events, warm clocks, one process).  One JSON line per
shape:

    evaluator  10 000 surface samples against a mesh of 320 000 faces 3 mm away: 30 000 slots on 160 002 vertices, short runs
    smpl       1 000 000 points within 0.1 m of a 13 776-face body: 3 000 000 slots on 6 890 vertices, runs of hundreds of slots

Legs, interleaved:
    forward          Mesh.closest (all four outputs): what a training step pays before the backward
    backward         Mesh.closest_backward, dpts and dverts
    backward_dpts    the same call with dpts alone (no keys, no sort, no runs): the difference to `backward` is the scatter's cost
    backward_attr3   dpts, dverts and dattr with C = 3
    torch_index_add  the same dpts and dverts written in torch: 2 g (p - q), then index_add_ of -(b_k dpts) onto the vertices — float
                     atomics and the framework's kernels, the path this entry replaces; its bits change from run to run

    python tools/bench_mesh_closest_grad.py [--out profiles/mesh_closest_grad.jsonl] [--reps 10]

The line carries a checksum of dverts' bits and whether a second call repeats them.
No time is asserted.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_mesh_distance import SCALE, stats, subdivide, template, timed
from relightableavatar_amd import mesh_utils
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def run_shape(eng, name, verts, faces, pts, reps, note):
    dev = eng.device
    tv, tf = torch.from_numpy(verts.astype(np.float32)).to(dev), torch.from_numpy(faces.astype(np.int32))
    pts = pts.to(dev).float().contiguous()
    n, V = pts.shape[0], tv.shape[0]
    mesh = eng.mesh(tv, tf)
    out = mesh.closest(pts)
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn(n, device=dev, generator=gen)
    ga = torch.randn(n, 3, device=dev, generator=gen)
    corners = mesh.faces_device().long()[out.face.long()].reshape(-1)

    def torch_leg():
        dpts = (2 * g)[:, None] * (pts - out.closest)
        return dpts, torch.zeros(V, 3, device=dev).index_add_(0, corners, (-(out.bary[..., None] * dpts[:, None])).reshape(-1, 3))

    legs = {'forward': lambda: mesh.closest(pts),
            'backward': lambda: mesh.closest_backward(pts, out, g, want=('dpts', 'dverts')),
            'backward_dpts': lambda: mesh.closest_backward(pts, out, g, want=('dpts',)),
            'backward_attr3': lambda: mesh.closest_backward(pts, out, g, ga),
            'torch_index_add': torch_leg}
    for fn in legs.values():         # warm-up of every leg: code objects, ctx scratch, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    ours, theirs = legs['backward'](), torch_leg()
    again = legs['backward']()
    slots = torch.bincount(corners, minlength=V)
    line = dict(tool='bench_mesh_closest_grad', shape=name, note=note, faces=int(len(faces)), verts=int(V), points=int(n), reps=reps,
                device=torch.cuda.get_device_name(0),
                slots_per_vertex_max=int(slots.max()), vertices_with_slots=int((slots > 0).sum()),
                repeatable=bool(torch.equal(ours.dverts.view(torch.int32), again.dverts.view(torch.int32))),
                dverts_bits_crc32=zlib.crc32(ours.dverts.cpu().numpy().tobytes()),
                dverts_max_abs_diff_to_torch=float((ours.dverts - theirs[1]).abs().max()), dverts_max_abs=float(ours.dverts.abs().max()))
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    for k in t:
        stats(line, k, t[k])
    line['scatter_ms'] = round(line['backward_ms'] - line['backward_dpts_ms'], 4)
    line['torch_over_backward'] = round(line['torch_index_add_ms'] / line['backward_ms'], 2)
    mesh.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'mesh_closest_grad.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--smpl-points', type=int, default=1000000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    gen = torch.Generator().manual_seed(0)
    lines = []
    # bench_mesh_distance's two shapes, drawn the same way
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    src = torch.from_numpy(v * SCALE * (1 + 0.003 / SCALE.mean()))
    pts = mesh_utils.sample_surface(src, torch.from_numpy(f), 10000, gen)[0]
    lines.append(run_shape(eng, 'evaluator', v * SCALE, f, pts, args.reps, '10 000 surface samples, 3 mm from the mesh'))
    v, f = template(6890)
    on = mesh_utils.sample_surface(torch.from_numpy(v * SCALE), torch.from_numpy(f), args.smpl_points, gen)[0]
    off = torch.randn(args.smpl_points, 3, generator=gen, dtype=torch.float64)
    off = off / off.norm(dim=-1, keepdim=True) * 0.1 * torch.rand(args.smpl_points, 1, generator=gen, dtype=torch.float64)
    lines.append(run_shape(eng, 'smpl', v * SCALE, f, on + off, args.reps, 'points within 0.1 m of the surface'))
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

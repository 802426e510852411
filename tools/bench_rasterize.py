"""ra_rasterize / ra_interpolate and their backward passes: time per call (HIP events, warm clocks, one process).  One JSON line per
shape:

    camera320k   512 x 512 pixels, a pinhole 3 m in front of a mesh of 320 000 faces (the synthetic template at 2 502 vertices,
                 subdivided three times onto its ellipsoid): bench_mesh_raycast's camera shape, sampled at the pixel centres
    body13776    the same camera on the 13 776-face hull of the 6 890-vertex template (SMPL's counts)

Legs, all for a NEW POSE (nothing of an earlier call is reused):
    raster            Engine.rasterize, then Engine.interpolate of 3 channels — the forward of a rendered attribute map
    rasterize, interpolate, brute   its parts, and the RA_RASTER_BRUTE scan (which must return the same bits; the line says so)
    raycast_new_pose  what the tree could do before: Engine.mesh (ra_mesh_create: the box structure of this pose) plus Mesh.raycast
                      with RA_RAYCAST_UNSORTED for t, face, uv through the same pixel centres
    raycast           that raycast alone, on a mesh built before
    backward          Engine.interpolate_backward (d attr, d uv) then Engine.rasterize_backward (d pos)

    python tools/bench_rasterize.py [--out profiles/rasterize.jsonl] [--reps 10]

Every leg is warmed up (code objects, ctx scratch, clocks), then timed `reps` times, the legs interleaved; the median and min .. max
are reported.  No target is fixed here: the numbers are written down (DESIGN.md section 25 compares raster with raycast_new_pose).
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
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine

FOV, DIST = 0.55, 3.0        # bench_mesh_raycast's camera: at (0, -3, 0), looking along +y, x right, z up


def run_shape(eng, name, verts, faces, H, reps, with_brute, note):
    dev = eng.device
    tv = torch.from_numpy(verts.astype(np.float32)).to(dev)
    tf_host = torch.from_numpy(faces.astype(np.int32))
    tf = tf_host.to(dev)
    s = DIST / FOV
    pos = torch.stack([tv[:, 0] * s, -tv[:, 2] * s, torch.full_like(tv[:, 0], -0.02), tv[:, 1] + DIST], -1)[None].contiguous()
    px = (torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1
    gz, gx = torch.meshgrid(px, px, indexing='ij')
    d = torch.stack([gx * FOV, torch.full_like(gx, DIST), -gz * FOV], -1).reshape(-1, 3).to(dev).float().contiguous()
    o = torch.tensor([0.0, -DIST, 0.0], device=dev).expand_as(d).contiguous()
    attrs = torch.rand(tv.shape[0], 3, device=dev)
    topo = eng.topology(tf, tv.shape[0])
    mesh = eng.mesh(tv, tf_host)

    def raycast_new_pose():
        m = eng.mesh(tv, tf_host)
        out = m.raycast(o, d, want=('t', 'face', 'uv'), sort=False)
        m.close()
        return out

    rast = eng.rasterize(pos, tf, H, H)
    dout, duv = torch.rand(1, H, H, 3, device=dev), torch.rand(1, H, H, 2, device=dev)

    def backward():
        g = eng.interpolate_backward(topo, attrs, rast, dout)
        return eng.rasterize_backward(topo, pos, rast, g.duv + duv)

    legs = {'raster': lambda: eng.interpolate(attrs, eng.rasterize(pos, tf, H, H), tf), 'rasterize': lambda: eng.rasterize(pos, tf, H, H),
            'interpolate': lambda: eng.interpolate(attrs, rast, tf), 'raycast_new_pose': raycast_new_pose,
            'raycast': lambda: mesh.raycast(o, d, want=('t', 'face', 'uv'), sort=False), 'backward': backward}
    if with_brute:
        legs['brute'] = lambda: eng.rasterize(pos, tf, H, H, brute=True)
    for fn in legs.values():         # warm-up of every leg
        fn()
    torch.cuda.synchronize()
    line = dict(tool='bench_rasterize', shape=name, note=note, faces=int(len(faces)), verts=int(len(verts)), image=[H, H], reps=reps,
                device=torch.cuda.get_device_name(0), covered_share=float((rast.face >= 0).float().mean()))
    if with_brute:
        b = eng.rasterize(pos, tf, H, H, brute=True)
        line['brute_bit_identical'] = bool(all(torch.equal(rast[k].view(torch.int32), b[k].view(torch.int32)) for k in ('uv', 'zw', 'face')))
    ray = mesh.raycast(o, d, want=('face',), sort=False).face.view(H, H)
    line['raycast_face_differs_on'] = int((ray != rast.face[0]).sum())
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    for k in t:
        stats(line, k, t[k])
    line['raster_over_raycast_new_pose'] = round(line['raster_ms'] / line['raycast_new_pose_ms'], 3)
    mesh.close()
    topo.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'rasterize.jsonl'))
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
    lines.append(run_shape(eng, 'camera320k', v * SCALE, f, args.image, args.reps, False, f'{args.image} x {args.image} pixels from 3 m, {len(f)} faces'))
    v, f = template(6890)
    lines.append(run_shape(eng, 'body13776', v * SCALE, f, args.image, args.reps, True, f'{args.image} x {args.image} pixels from 3 m, {len(f)} faces'))
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

"""Times ra_mesh_winding (Mesh.winding) and one full winding-distance remesh on the device.

    python tools/bench_winding.py [--reps 5] [--out profiles/winding.jsonl] [--quick]

1. Pairs per second of the kernel at four (points, faces) sizes on the synthetic hull — a grid band against a scan (3e5 x 5e5), the
   same points against a template-sized mesh, few points against many faces (the split launch) and its one-pass shape beside it — with
   the useful VALU rate that goes with it: PAIR_OPS vector instructions per pair, counted in the kernel's ISA, over the chip's issue
   rate.  The kernel moves next to no memory (a 48-byte face record per wave and pair through the scalar cache), so the bound is VALU
   issue; the share printed is of that.
2. For orientation, the same formula as dense torch operations on the device (the reference's form, in row chunks that fit memory), at
   the one size where that is affordable.
3. One winding_distance_remesh of a 20 000-face hull at voxel 0.01, timed per stage with the stages run by hand.
Host clock around calls that end in a device synchronise, one warm-up call per shape, the median of --reps with min .. max.  One JSON
line per measurement.  No speed is promised anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from relightableavatar_amd import mesh_utils, synthetic                    # noqa: E402
from relightableavatar_amd.config import make_cfg                           # noqa: E402

PAIR_OPS = 184                    # vector instructions per (point, face) pair in winding_kernel's loop body (gfx950 ISA of this build; 10 of them
                                  # reciprocals and square roots, which hold the issue port twice as long)
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9      # CUs x SIMDs x lanes per cycle x clock: one vector instruction per lane


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def hull(n_verts):
    b = synthetic.make_body(0, posed=False, n_verts=n_verts)
    tv = b.tverts[0].numpy()
    return tv, synthetic._template_faces(tv.astype(np.float64) / (0.4 * np.array([0.8, 0.7, 1.1])))


def band_points(v, n, seed=0):
    """n points within 5 mm of the hull's vertices: what the remesh's filters leave"""
    g = np.random.default_rng(seed)
    return (v[g.integers(0, len(v), n)] + g.normal(0, 0.003, (n, 3))).astype(np.float32)


def dense_torch(pts, verts, faces, rows):
    """the reference's formula as dense torch operations, in chunks of rows"""
    tri = verts[faces.long()]
    out = []
    for i in range(0, len(pts), rows):
        u = tri[None] - pts[i:i + rows, None, None, :]
        u = u / u.norm(dim=-1, keepdim=True)
        u0, u1, u2 = u[:, :, 0], u[:, :, 1], u[:, :, 2]
        e0, e1, e2 = u1 - u0, u2 - u1, u0 - u2
        sign = (torch.linalg.cross(e0, e1) * u2).sum(-1).sign()
        l = 2 * (torch.stack([e0.norm(dim=-1), e1.norm(dim=-1), e2.norm(dim=-1)], -1) / 2).arcsin()
        s = l.sum(-1) / 2
        t = (s / 2).tan() * ((s - l[..., 0]) / 2).tan() * ((s - l[..., 1]) / 2).tan() * ((s - l[..., 2]) / 2).tan()
        out.append(((4 * (t.abs() + 1e-10).sqrt().arctan()) * sign).sum(-1) / (4 * torch.pi))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    ap.add_argument('--quick', action='store_true', help='a tenth of the sizes: a rehearsal of the tool, not a measurement')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_winding needs an MI355X'
    from relightableavatar_amd.engine import Engine
    dev = torch.device('cuda:0')
    eng = Engine(make_cfg('relight'), device='cuda:0')
    q = 10 if a.quick else 1
    lines = []

    def emit(**kw):
        kw.update(tool='bench_winding', reps=a.reps, quick=a.quick, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    meshes = {}
    for n_verts in sorted({250001 // q, 3501}):
        v, f = hull(n_verts)
        meshes[len(f)] = (v, torch.from_numpy(v).to(dev), f, eng.mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f)))
    big, small = max(meshes), min(meshes)
    for n, n_faces, shape in ((300000 // q, big, None), (300000 // q, small, None), (256, big, None), (256, big, 'one_pass'), (16384, big, None)):
        v, tv, f, mesh = meshes[n_faces]
        p = torch.from_numpy(band_points(v, n)).to(dev)
        _, t = timed(lambda: mesh.winding(p, shape=shape), a.reps)
        pairs = n * n_faces
        rate = pairs / (t['median_ms'] * 1e-3)
        emit(what='ra_mesh_winding', points=n, faces=n_faces, shape=shape or 'default', pairs=pairs, pairs_per_s=rate,
             valu_ops_per_pair=PAIR_OPS, share_of_valu_issue=round(rate * PAIR_OPS / PEAK_LANE_OPS, 4), **t)
    # orientation: dense torch on the device at the small mesh
    v, tv, f, mesh = meshes[small]
    n = 20000 // q
    p = torch.from_numpy(band_points(v, n)).to(dev)
    tf = torch.from_numpy(f).to(dev)
    rows = max(1, int(2 ** 28 // (len(f) * 9)))
    dense, t = timed(lambda: dense_torch(p, tv, tf, rows), max(1, a.reps // 2))
    w, tk = timed(lambda: mesh.winding(p), a.reps)
    emit(what='dense torch beside the kernel', points=n, faces=len(f), rows_per_chunk=rows, dense_torch=t, kernel=tk,
         dense_pairs_per_s=n * len(f) / (t['median_ms'] * 1e-3), kernel_pairs_per_s=n * len(f) / (tk['median_ms'] * 1e-3),
         max_abs_diff=float((dense - w).abs().max()))
    # one remesh, per stage
    n_verts = 10001 // q
    v, f = hull(n_verts)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f)
    vs, th_v, th_t = 0.01, 0.05, 0.02
    (pts, wb), t_grid = timed(lambda: mesh_utils.get_voxel_grid_and_update_bounds([vs] * 3, mesh_utils.get_bounds(tv[None], th_t)), a.reps)
    sh, pts = pts.shape[1:-1], pts.view(-1, 3)
    d1, t_l1 = timed(lambda: mesh_utils.sample_closest_points(pts[None], tv[None])[0, :, 0], a.reps)
    p1 = pts[d1 < th_v]
    mesh, t_build = timed(lambda: eng.mesh(tv, tf), a.reps)
    d, t_l2 = timed(lambda: mesh.closest(p1, want=('d2',)).d2.sqrt(), a.reps)
    p2, d2 = p1[d < th_t], d[d < th_t]
    w, t_w = timed(lambda: mesh.winding(p2), a.reps)
    cube = torch.full((pts.shape[0],), -10.0, device=dev)
    cube[torch.nonzero(d1 < th_v)[:, 0][d < th_t]] = mesh_utils.winding_shift(w, 0.5, 0.75) * d2
    cube = cube.view(*sh)
    (mv, mf), t_mc = timed(lambda: eng.marching_cubes(cube, 0.0), a.reps)
    (ov, of), t_cc = timed(lambda: eng.largest_component(mv, mf), a.reps)
    _, t_all = timed(lambda: mesh_utils.winding_distance_remesh(tv, tf, voxel_size=vs, dist_th_verts=th_v, dist_th_tris=th_t, engine=eng), a.reps)
    emit(what='winding_distance_remesh', faces=len(f), voxel_size=vs, grid_shape=list(sh), grid_points=int(pts.shape[0]), after_vertex_filter=int(p1.shape[0]),
         after_surface_filter=int(p2.shape[0]), winding_pairs=int(p2.shape[0]) * len(f), out_verts=int(ov.shape[0]), out_faces=int(of.shape[0]),
         grid=t_grid, vertex_filter=t_l1, mesh_build=t_build, surface_filter=t_l2, winding=t_w, marching_cubes=t_mc, largest_component=t_cc, whole=t_all)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

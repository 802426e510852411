"""Times ra_mesh_winding_grad (Mesh.winding_grad) and one isosurface fit on the device.

    python tools/bench_winding_grad.py [--reps 5] [--out profiles/winding_grad.jsonl] [--quick] [--legs value,grad,autograd,fit] [--repo DIR]

1. `grad`: the gradient kernel at the two shapes a fit and a field evaluation give it — 1 600 points against 499 998 faces (the split
   launch) and 300 000 points against 598 faces (the one-pass kernel) — in pairs per second, with the useful VALU rate that goes with
   it: PAIR_OPS vector instructions per pair, counted in the split kernel's loop body in the ISA, over the chip's issue rate.  Like
   the value kernel it moves next to no memory: the bound is VALU issue, and the share printed is of that.
2. `value`: ra_mesh_winding alone at the same shapes and points.  --repo DIR imports the package from another checkout (the parent
   commit's tree, built): this leg calls nothing that tree lacks.
3. `autograd`: for orientation, the reference's formula as dense torch operations under torch.autograd on the device, forward and
   backward in row chunks that fit memory, at 1 600 points against 19 998 faces, with the kernel beside it at that shape.
4. `fit`: the wall time of one 100-iteration isosurface_fitting at its defaults: a 7 000-face source, 1 600 of its vertices per
   iteration, against the 499 998-face target.
Host clock around calls that end in a device synchronise, one warm-up call per shape, the median of --reps with min .. max.  One JSON
line per measurement.  No speed is promised anywhere."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

PAIR_OPS = 287                    # vector instructions per (point, face) pair in winding_grad_split_kernel's loop body (gfx950 ISA of this build;
                                  # 14 of them reciprocals and square roots, 8 float64)
VALUE_PAIR_OPS = 184              # tools/bench_winding.py's count for the value kernel
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9      # CUs x SIMDs x lanes per cycle x clock: one vector instruction per lane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    ap.add_argument('--quick', action='store_true', help='a tenth of the sizes: a rehearsal of the tool, not a measurement')
    ap.add_argument('--legs', default='value,grad,autograd,fit')
    ap.add_argument('--repo', default=os.path.dirname(HERE), help='the checkout whose package and library are timed (default: this one)')
    a = ap.parse_args()
    legs = a.legs.split(',')
    library = 'this checkout' if os.path.abspath(a.repo) == os.path.dirname(HERE) else 'another checkout (--repo)'
    assert set(legs) <= {'value', 'grad', 'autograd', 'fit'}, legs
    sys.path.insert(0, os.path.abspath(a.repo))
    from relightableavatar_amd import mesh_utils                                # noqa: E402  (before bench_winding, which would put its own tree first)
    from relightableavatar_amd.config import make_cfg                           # noqa: E402
    from relightableavatar_amd.engine import Engine                             # noqa: E402
    sys.path.insert(0, HERE)
    from bench_winding import band_points, dense_torch, hull, timed             # noqa: E402
    assert torch.cuda.is_available(), 'bench_winding_grad needs an MI355X'
    dev = torch.device('cuda:0')
    eng = Engine(make_cfg('relight'), device='cuda:0')
    q = 10 if a.quick else 1
    lines = []

    def emit(**kw):
        kw.update(tool='bench_winding_grad', reps=a.reps, quick=a.quick, device=torch.cuda.get_device_name(0), library=library)
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    meshes = {}
    for n_verts in (250001 // q, 301):
        v, f = hull(n_verts)
        meshes[len(f)] = (v, torch.from_numpy(v).to(dev), f, eng.mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f)))
    big, small = max(meshes), min(meshes)
    for n, n_faces, shape in ((1600, big, 'split'), (300000 // q, small, 'one_pass')):
        v, tv, f, mesh = meshes[n_faces]
        p = torch.from_numpy(band_points(v, n)).to(dev)
        pairs = n * n_faces
        for leg, fn, ops in (('value', lambda: mesh.winding(p), VALUE_PAIR_OPS), ('grad', lambda: mesh.winding_grad(p), PAIR_OPS)):
            if leg not in legs:
                continue
            _, t = timed(fn, a.reps)
            rate = pairs / (t['median_ms'] * 1e-3)
            emit(what='ra_mesh_winding_grad' if leg == 'grad' else 'ra_mesh_winding', points=n, faces=n_faces, shape=f'default ({shape})', pairs=pairs,
                 pairs_per_s=rate, valu_ops_per_pair=ops, share_of_valu_issue=round(rate * ops / PEAK_LANE_OPS, 4), **t)
    if 'autograd' in legs:
        v, f = hull(10001 // q)
        tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        p = torch.from_numpy(band_points(v, 1600)).to(dev)
        rows = max(1, int(2 ** 27 // (len(f) * 9)))          # autograd keeps the forward's tensors: half of bench_winding's chunk

        def dense_backward():
            g = []
            for i in range(0, len(p), rows):
                x = p[i:i + rows].clone().requires_grad_()
                dense_torch(x, tv, tf, rows).sum().backward()
                g.append(x.grad)
            return torch.cat(g)

        mesh = eng.mesh(tv, torch.from_numpy(f))
        dense, t = timed(dense_backward, max(1, a.reps // 2))
        (w, g), tk = timed(lambda: mesh.winding_grad(p), a.reps)
        scale, fin = float(g.abs().max()), torch.isfinite(dense).all(1)
        emit(what='dense torch autograd beside the kernel', points=len(p), faces=len(f), rows_per_chunk=rows, dense_torch_autograd=t, kernel=tk,
             max_abs_diff_over_max_abs_grad=float((dense - g)[fin].abs().max()) / scale, dense_rows_not_finite=int((~fin).sum()))
    if 'fit' in legs:
        sv, sf = hull(3501 // q)
        c = sv.mean(0, dtype=np.float64)
        src = torch.from_numpy((c + 1.05 * (sv.astype(np.float64) - c)).astype(np.float32)).to(dev)
        v, tv, f, _ = meshes[big]
        gen = torch.Generator(device='cuda:0')

        def fit():
            gen.manual_seed(0)
            return mesh_utils.isosurface_fitting(src, torch.from_numpy(sf), tv, torch.from_numpy(f), generator=gen, engine=eng)

        out, t = timed(fit, max(1, a.reps // 2))
        emit(what='isosurface_fitting', f='winding_distance', thresh=0.5, opt_iter=100, chunk_size=1600, src_verts=len(sv), src_faces=len(sf), target_faces=len(f),
             pairs_per_iteration=min(1600, len(sv)) * len(f), largest_move=float((out - src).norm(dim=-1).max()), **t)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

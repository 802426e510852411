"""One cloth_energy forward plus gradient (stretch + bending + gravity) on a Loop-subdivided sphere of about 40 k vertices, at B = 1 and
8: HIP events around windows of `--inner` warm calls (a single call is tens of microseconds: one call per window would time the
clock), the time per call reported, one process.  One JSON line per batch size.

Beside it goes the same energy written in torch operations — the float32 restatement of tests/physx_ref.py (torch_energy) on the same
device, forward plus its autograd backward — for scale; the two results are compared and the line says by how much they differ.  The
library's parts (energies only; each term's forward plus gradient) are timed as well.

    python tools/bench_cloth.py [--out profiles/cloth.jsonl] [--reps 20] [--warmup 5] [--inner 20]

No ratio is fixed in advance: the numbers are written down.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import physx_ref as P
from bench_mesh_distance import SCALE, stats, template, timed
from relightableavatar_amd import physx_utils
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'cloth.jsonl'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--subdivisions', type=int, default=2)
    ap.add_argument('--inner', type=int, default=20, help='calls per timed window')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    dev = eng.device
    v, f = template(2502)
    tv, tf = torch.from_numpy((v * SCALE).astype(np.float32)).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    topo = eng.topology(tf, tv.shape[0])
    for _ in range(args.subdivisions):
        tv, tf, topo = topo.subdivide(tv)
    vm, fm = (torch.from_numpy(a) for a in P.flatten_faces(tv.cpu().double().numpy(), tf.cpu().long().numpy()))
    g = physx_utils.Garment(tv, tf, vm, fm, physx_utils.StVKMaterial(), engine=eng)
    V, F, H = tv.shape[0], tf.shape[0], g.f_connectivity.shape[0]
    print(f'mesh: {V} vertices, {F} faces, {H} hinges', file=sys.stderr, flush=True)
    tg = dict(f=g.f, ef=g.f_connectivity, ev=g.f_connectivity_edges, f_area=g.f_area, Dm_inv=g.Dm_inv, v_mass=g.v_mass, material=P.material())
    all3 = ('stretch', 'bending', 'gravity')
    lines = []
    for B in (1, 8):
        gen = torch.Generator(device='cpu').manual_seed(B)
        x = (tv[None] + (torch.rand(B, V, 3, generator=gen) * 0.004 - 0.002).to(dev)).contiguous()

        def lib_step():
            return g.cloth.energy(x, terms=all3)

        def torch_step():
            y = x.clone().requires_grad_()
            e = P.torch_energy(y, tg, stretch=True, bending=True, gravity=True)
            e.backward()
            return e, y.grad

        e, grad = lib_step()
        et, gt = torch_step()
        legs = {k: [] for k in ('lib', 'torch', 'lib_energy_only', 'lib_stretch', 'lib_bending', 'lib_gravity')}
        for k in range(args.warmup + args.reps):
            rec = k >= args.warmup
            for name, fn in (('lib', lib_step), ('torch', torch_step), ('lib_energy_only', lambda: g.cloth.energy(x, terms=all3, grad=False)),
                             ('lib_stretch', lambda: g.cloth.energy(x, terms=('stretch',))), ('lib_bending', lambda: g.cloth.energy(x, terms=('bending',))),
                             ('lib_gravity', lambda: g.cloth.energy(x, terms=('gravity',)))):
                t = timed(lambda: [fn() for _ in range(args.inner)]) / args.inner
                if rec:
                    legs[name].append(t)
        line = dict(tool='bench_cloth', verts=V, faces=F, hinges=H, B=B, terms=list(all3), reps=args.reps, warmup=args.warmup, calls_per_window=args.inner,
                    device=torch.cuda.get_device_name(0), hip=torch.version.hip, clock='device events around a window of calls, per call, median of the windows', energy=float(e.sum()) / B, energy_torch=float(et.detach()),
                    energy_rel_diff=abs(float(e.sum()) / B - float(et.detach())) / abs(float(et.detach())),
                    grad_rel_diff=float((grad / B - gt).abs().max() / gt.abs().max()))
        for k in legs:
            stats(line, k, legs[k])
        line['torch_over_lib'] = round(line['torch_ms'] / line['lib_ms'], 2)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

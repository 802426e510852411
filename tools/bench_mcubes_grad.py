"""Times the backward of marching cubes beside its forward on bench_mesh_extract.py's volume (synthetic.make_body, T-pose mode,
voxel_size 0.005, -sdf = 0).

    python tools/bench_mcubes_grad.py [--reps 10] [--out profiles/mcubes_grad.jsonl]

Legs: Engine.marching_cubes (classify, sum, ONE blocking read-back, emit), the backward with dvolume alone (classify, sum, gather; no
read-back), the backward with 3 attribute channels (dvolume and dattrs), the attribute forward with 3 channels.  HIP events around every
call, every leg warmed, --reps repetitions with the legs interleaved; per leg the median and min .. max.  Prints one JSON line.
`backward_within_forward` says whether the dvolume-alone backward's median is at most the forward's in this run."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from relightableavatar_amd import data_utils, synthetic                    # noqa: E402
from relightableavatar_amd.config import make_cfg                           # noqa: E402
from relightableavatar_amd.networks import make_network                     # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mcubes_grad needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = make_cfg('relight')
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
    net = net.to(dev).eval()
    body = synthetic.make_body(0, posed=True)
    eng = net.set_frame(synthetic.to_device(body, dev))
    axes = data_utils.mesh_grid_axes(body['tbounds'][0], [0.005] * 3)
    vol = eng.sdf_volume(*axes, 'tpose', cfg.dist_th)
    verts, faces = eng.marching_cubes(vol, 0.0)
    V = verts.shape[0]
    gen = torch.Generator(device=dev).manual_seed(0)
    dverts = torch.randn(V, 3, device=dev, generator=gen)
    attrs = torch.rand(vol.numel(), 3, device=dev, generator=gen)
    dattr = torch.randn(V, 3, device=dev, generator=gen)
    legs = {
        'marching_cubes': lambda: eng.marching_cubes(vol, 0.0),
        'backward_dvolume': lambda: eng.marching_cubes_backward(vol, 0.0, V, dverts=dverts, want=('dvolume',)),
        'backward_attrs3': lambda: eng.marching_cubes_backward(vol, 0.0, V, dverts=dverts, attrs=attrs, dattr=dattr),
        'attrs_forward3': lambda: eng.marching_cubes_attrs(vol, 0.0, attrs, V),
    }
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(event_ms(fn))
    stat = lambda t: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    res = dict(tool='bench_mcubes_grad', volume=list(vol.shape), points=int(vol.numel()), verts=int(V), faces=int(faces.shape[0]),
               **{k: stat(t) for k, t in ts.items()}, reps=a.reps, device=torch.cuda.get_device_name(0))
    res['backward_within_forward'] = bool(res['backward_dvolume']['median_ms'] <= res['marching_cubes']['median_ms'])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

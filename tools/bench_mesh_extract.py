"""Times one mesh extraction on the device, per stage, at voxel_size 0.005 on synthetic.make_body with synthetic weights: the volume
(Engine.sdf_volume, T-pose mode: K-NN filter, compaction, the compensated decoder, scatter), marching cubes at -sdf = 0 and the largest
component.

    python tools/bench_mesh_extract.py [--reps 5] [--out profiles/mesh_extract.jsonl]

Per stage: host clock around a call that ends in its own blocking read-back and a device synchronise, one warm-up call, the median of
--reps with min .. max.  Prints one JSON line with the blocking read-backs of every stage and of the whole extraction, which must not
exceed three (kept points, vertex / face counts, component result).  No time is promised anywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from relightableavatar_amd import data_utils, synthetic                    # noqa: E402
from relightableavatar_amd.config import make_cfg                           # noqa: E402
from relightableavatar_amd.networks import make_network                     # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_extract needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = make_cfg('relight')
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
    net = net.to(dev).eval()
    body = synthetic.make_body(0, posed=True)
    eng = net.set_frame(synthetic.to_device(body, dev))
    axes = data_utils.mesh_grid_axes(body['tbounds'][0], [0.005] * 3)
    vol, t_vol = timed(lambda: eng.sdf_volume(*axes, 'tpose', cfg.dist_th), a.reps)
    kept = eng.last_kept
    (v, f), t_mc = timed(lambda: eng.marching_cubes(vol, 0.0), a.reps)
    (ov, of), t_cc = timed(lambda: eng.largest_component(v, f), a.reps)
    # counted by the library where it synchronises behind a device-to-host copy, per entry point, for the last call of each
    stats = lambda k: int(eng.lib.ra_mesh_extract_stats(eng.ctx, k))
    readbacks = dict(sdf_volume=stats(0), marching_cubes=stats(1), largest_component=stats(2))
    readbacks['extraction'] = sum(readbacks.values())
    assert readbacks['extraction'] <= 3, readbacks
    res = dict(tool='bench_mesh_extract', grid=[len(x) for x in axes], volume=list(vol.shape), points=int(vol.numel()), kept_points=int(kept),
               verts=int(v.shape[0]), faces=int(f.shape[0]), kept_verts=int(ov.shape[0]), kept_faces=int(of.shape[0]), sdf_volume=t_vol,
               marching_cubes=t_mc, largest_component=t_cc, blocking_readbacks=readbacks,
               label_passes=stats(3), label_passes_queued=int(eng.lib.ra_mcubes_tile(1)), reps=a.reps,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

"""ra_reshade and ra_reshade_backward on the same inputs: time per call (HIP events, warm clocks, one process) at P = 20 000 (the
headline frame's hit pixels) and P = 262 144, with 1 and 8 probes.  One JSON line per shape.

    python tools/bench_reshade_backward.py [--out profiles/reshade_backward.jsonl] [--shape P,N ...] [--reps 20]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_reshade_backward.py --out /dev/null --reps 5      # kernel shares, a run of its own

Each shape: both calls warmed up (every shape loads its code objects and grows the ctx scratch on its first call), then `reps` timed
repetitions of each, interleaved; the median and the spread are reported.  The backward is judged against the forward of the same run
(`ratio`).  Arithmetic per (pixel, light): the backward evaluates the BRDF twice (pass 1 sums lin like the forward, pass 2 adds the
roughness derivative) and the probe lookup twice, and adds 12 LDS float adds per probe: > 2 x the forward is expected before the
reduction.  The share of the cross-workgroup reduction (slab_sum_kernel) comes from the kernel trace, not from this script.
A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from relightableavatar_amd import synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.networks import make_network


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'reshade_backward.jsonl'))
    ap.add_argument('--shape', action='append', help='P,n_probes (default: 20000,1 20000,8 262144,1 262144,8)')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(',')) for s in (args.shape or ['20000,1', '20000,8', '262144,1', '262144,8'])]
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = make_cfg('relight')
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
    net = net.to(dev).eval()
    eng = net.set_frame(synthetic.to_device(synthetic.make_body(0, posed=True), dev))
    lines = []
    for P, n in shapes:
        x = synthetic.make_reshade_inputs(60, P, n_probes=n, rough=(0.09, 0.99))
        x = {k: v.to(dev) for k, v in x.items()}
        a = (x['ray_o'], x['surf'], x['norm'], x['albedo'], x['rough'], x['lvis'], x['ldot'], x['probes'])
        fwd = lambda: eng.reshade(*a, want_spec=False)
        bwd = lambda: eng.reshade_backward(*a, x['d_rgb'])
        bwd_np = lambda: eng.reshade_backward(*a, x['d_rgb'], want=(True, True, False))
        for _ in range(3):           # warm-up: code objects, scratch, clocks
            fwd(), bwd(), bwd_np()
        torch.cuda.synchronize()
        t = {'forward': [], 'backward': [], 'backward_no_probe': []}
        for _ in range(args.reps):   # interleaved: the three see the same clocks
            for name, fn in (('forward', fwd), ('backward', bwd), ('backward_no_probe', bwd_np)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1))
        r = dict(tool='bench_reshade_backward', P=P, n_probes=n, lights=cfg.env_h * cfg.env_w, probe=[int(x['probes'].shape[1]), int(x['probes'].shape[2])],
                 reps=args.reps, device=torch.cuda.get_device_name(0))
        for k, v in t.items():
            r[k + '_ms'] = round(median(v), 4)
            r[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        r['ratio'] = round(r['backward_ms'] / r['forward_ms'], 3)
        r['ratio_no_probe'] = round(r['backward_no_probe_ms'] / r['forward_ms'], 3)
        r['note'] = 'times include the allocation of the outputs by the host framework (both calls alike); HIP events around one call'
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if args.out and args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

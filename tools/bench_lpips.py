"""ra_lpips on one 512 x 512 relit frame against a perturbed copy: time per call (HIP events, warm clocks, one process).  Three JSON lines:

    1  one Engine.lpips call on the frame's ray list (the in-box rays of the render), and on the assembled full image
    2  N = 8 calls back to back into one (8, 6) table, plus the one device-to-host copy of the table (what Evaluator.summarize does)
    3  for context only: the host path a user has without it — both ray lists copied to the host, the images assembled, and the float32
       torch-CPU restatement of the metric (tests/lpips_ref.py; the lpips package itself is not a dependency of this project), wall clock

    python tools/bench_lpips.py [--out profiles/lpips.jsonl] [--size 512] [--reps 20]

The weights are the seeded synthetic set of tests/lpips_ref.py: the cost does not depend on their values.  Every leg is warmed up (code
objects, ctx scratch, clocks), then `reps` timed repetitions, the device legs interleaved; the median and the spread are reported.  No
target is fixed: the numbers are written down.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

import image_metrics_ref as IM
import lpips_ref as R
from relightableavatar_amd import synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.networks import make_network
from relightableavatar_amd.renderer import make_renderer


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lpips.jsonl'))
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda:0')
    cfg = make_cfg('relight')
    net = make_network(cfg)
    net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
    net = net.to(dev).eval()
    H = W = args.size
    batch = synthetic.to_device(synthetic.make_batch(H, W, seed=0, posed=True), dev)
    out = make_renderer(cfg, net).render(batch)
    eng = net.engine()
    sd = R.weights(0)
    eng.lpips_load(sd)
    pred = out.rgb_map.reshape(-1, 3).contiguous()
    P = pred.shape[0]
    gt = (pred + 0.02 * torch.randn(pred.shape, generator=torch.Generator().manual_seed(0)).to(dev)).clamp(0, 1)
    pix = batch.mask_at_box[0].reshape(-1).nonzero()[:, 0].contiguous()
    assert pix.numel() == P
    bg = float(cfg.bg_brightness)
    full_p, full_g = torch.full((H * W, 3), bg, device=dev), torch.full((H * W, 3), bg, device=dev)
    full_p[pix], full_g[pix] = pred, gt
    table = torch.empty(args.frames, 6, dtype=torch.float64, device=dev)
    one_rays = lambda: eng.lpips(pred, gt, H, W, pix=pix, bg=bg, out=table[0])
    one_full = lambda: eng.lpips(full_p, full_g, H, W, bg=bg, out=table[0])

    def sequence():
        for k in range(args.frames):
            eng.lpips(pred, gt, H, W, pix=pix, bg=bg, out=table[k])
        return table.cpu()

    for _ in range(3):
        one_rays(), one_full(), sequence()
    torch.cuda.synchronize()
    t = {'ray_list': [], 'full_image': [], 'sequence': []}
    for _ in range(args.reps):
        for name, fn in (('ray_list', one_rays), ('full_image', one_full), ('sequence', sequence)):
            t[name].append(timed(fn))
    values = sequence()[0].tolist()
    common = dict(tool='bench_lpips', H=H, W=W, rays=P, reps=args.reps, device=torch.cuda.get_device_name(0), weights='synthetic, seed 0')
    l1 = dict(common, kind='one_call', values=dict(zip(('lpips', 'r0', 'r1', 'r2', 'r3', 'r4'), values)))
    stats(l1, 'ray_list', t['ray_list'])
    stats(l1, 'full_image', t['full_image'])
    l2 = dict(common, kind='sequence_into_one_table_plus_copy', frames=args.frames)
    stats(l2, 'sequence', t['sequence'])
    l2['per_frame_ms'] = round(l2['sequence_ms'] / args.frames, 4)

    def host_path():
        hp, hg, hpix = pred.cpu().numpy(), gt.cpu().numpy(), pix.cpu().numpy()
        ip, ig = IM.assemble(hp, hpix, H, W, bg), IM.assemble(hg, hpix, H, W, bg)
        return R.lpips(ip, ig, sd, torch.float32)[0]

    host_reps = max(3, args.reps // 4)
    host_path()
    th = []
    for _ in range(host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = host_path()
        th.append((time.perf_counter() - t0) * 1e3)
    l3 = dict(common, kind='host_path_for_context', reps=host_reps, clock='wall', cpu_threads=torch.get_num_threads(),
              note='device-to-host copy of both ray lists, assembly, the metric restated on torch-CPU in float32',
              values=dict(lpips=float(h[0])))
    stats(l3, 'host', th)
    with open(args.out, 'w') as f:
        for line in (l1, l2, l3):
            s = json.dumps(line)
            print(s)
            f.write(s + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Headline benchmark: rays/s for a 512x512 full-relight frame (16x32 light probe, DFSS visibility)
on synthetic weights, N GPUs of one node (one process per GPU, pixels dealt in 8x8 tiles, one RCCL
all_gather per frame).  Prints ONE JSON line on rank 0 (see the contract in the task statement).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--size 512] [--mode relight|sphere_tracing|anisdf|novel_light]
                    [--dump-outputs DIR] [--full]

A plain run sets up, soaks and warms up, times the K steps and prints the line (rays/s, ms_per_step, the roofline of the timed
steps).  `--full` adds the legs that take runs of their own: the CPU baseline and the PSNR against the oracle on its sample, the
strictly sequential frames (`ms_per_step_sequential`) and, with `--animate`, the same frames posed before the loop.
`--dump-outputs DIR` writes what the last timed step returned (DIR/<name>.npy, float32) for output-by-output comparisons of builds.

`--gpus N` with N > 1 outside a torchrun environment makes this process a LAUNCHER: it never touches the GPU, starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child (env:// rendezvous on 127.0.0.1, like the
reference's train.py:116-122), relays rank 0's JSON line and exits with the child's status.  Under torchrun (RANK set, the way
the driver starts it) the same file is the rank program.  `--backend gloo --dry` runs launcher + rank plumbing (process group,
shard plan, frame all_gather, barrier, MAX reduce, JSON line) on CPU tensors without the HIP engine: the CPU test of the N > 1 path.
"""
import argparse
import glob
import json
import math
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from relightableavatar_amd import synthetic, shard          # noqa: E402
from relightableavatar_amd.pipeline import FramePipeline    # noqa: E402
from relightableavatar_amd.base_utils import dotdict        # noqa: E402
from relightableavatar_amd.config import make_cfg           # noqa: E402
from relightableavatar_amd.networks import make_network     # noqa: E402
from relightableavatar_amd.renderer import make_renderer    # noqa: E402

F_SDF = 1_901_568          # algorithmic FLOP per fine distance query
F_FULL = 3_934_208 + 197_632
F_FULL_ANISDF = 3_934_208 + 541_184       # volume path: geometry point with normal + colour net
MFMA_PEAK_TFLOPS = 2500.0  # dense f16/bf16 MFMA peak, MI355X_MICROARCH.md


def cam_dist_of(coverage):
    """camera distance at which the synthetic body (a sphere of radius 0.4 m, focal length 0.8 H) covers `coverage` of the frame"""
    return 2.0 if coverage <= 0 else 0.8 * 0.4 / math.sqrt(coverage / math.pi)


# rays of the CPU leg's strided sample (about 3100: 10-20 s of oracle time on the GPU box's host cores since the oracle's K-NN works in
# cache-sized blocks — 1400 rays/s on 16 threads; rounds 1-4 and the first half of round 5 sampled 517 rays in 13 s)
N_SAMPLE = 3072


BODY_KW = {}          # --body split: synthetic.SPLIT_BODY_KW (a body part that shadows the body at distance)
WEIGHTS_KW = {}       # --weights sharp / --body split: make_state_dict(kind=, env=)


def sample_batch(H, skin_noise, n_target, cam_dist=2.0):
    """the bounded sample of the benchmarked frame: every stride-th of its in-box rays (rays are independent: one render chunk)."""
    return synthetic.sample_rays(synthetic.make_batch(H, H, seed=0, posed=True, skin_noise=skin_noise, cam_dist=cam_dist, **BODY_KW), n_target)


def fp32_unstable(net, batch, H, skin_noise, cam_dist, n_target):
    """rays of the sample whose traced surface the reference's own fp32 arithmetic does not pin (oracle.fp32_unstable_rays, tools/fp32_stability.py).
    The default samples' lists are committed (tests/golden/fp32_unstable_rays.json, 32 trials); any other sample is classified here with 8."""
    from oracle import ra_oracle as O
    case = {2.0: 'bench_sample_3072', 0.0: 'bench_sample_smooth_3072'}.get(float(skin_noise)) if (H == 512 and cam_dist == 2.0 and n_target == N_SAMPLE and not BODY_KW and not WEIGHTS_KW) else None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests', 'golden', 'fp32_unstable_rays.json')
    n = batch.ray_o.shape[1]
    if case and os.path.exists(path):
        d = json.load(open(path)).get(case)
        if d and d['n_rays'] == n:
            m = torch.zeros(n, dtype=torch.bool)
            m[d['unstable']] = True
            return m, f'tests/golden/fp32_unstable_rays.json:{case} (32 trials)'
    return O.fp32_unstable_rays(net, batch, trials=8), 'oracle.fp32_unstable_rays(trials=8) in this run'


def cpu_baseline(cfg, H, skin_noise, n_target=N_SAMPLE, threads=16, cam_dist=2.0):
    """oracle (CPU port of the reference path) on a strided sample of the same frame's rays.  Returns the bench line's
    `cpu_baseline` object and the oracle's maps of the sample (the checker of `psnr_vs_oracle`)."""
    from oracle import ra_oracle as O
    torch.set_num_threads(min(os.cpu_count() or 1, threads))   # more threads than this only add sync overhead here
    batch, P, stride = sample_batch(H, skin_noise, n_target, cam_dist)
    n = batch.ray_o.shape[1]
    net = O.OracleNet(synthetic.make_state_dict(0, relight=bool(cfg.relighting), cfg=cfg, **WEIGHTS_KW), cfg)
    t0 = time.perf_counter()
    if cfg.renderer_module.endswith('base_renderer'):
        ref = O.render_volume(net, batch)
    else:
        ref = O.render_sphere_tracing(net, batch)
    dt = time.perf_counter() - t0
    if not cfg.renderer_module.endswith('base_renderer'):        # (after the timed part) which of the sample's rays fp32 itself pins
        ref.fp32_unstable, ref.fp32_unstable_source = fp32_unstable(net, sample_batch(H, skin_noise, n_target, cam_dist)[0], H, skin_noise, cam_dist, n_target)
    # rays outside the body's bounding box cost nothing on either side: scale to whole-frame rays
    return dict(value=(n / P) * H * H / dt, unit='rays/s', cores=torch.get_num_threads(), kind='port',
                sample=f'every {stride}th of the {P} in-box rays of the same {H}x{H} frame ({n} rays, {dt:.1f} s), '
                       f'torch fp32 CPU restatement of the reference path (oracle/ra_oracle.py)'), ref


def psnr_vs_oracle(renderer, ref, H, skin_noise, dev, n_target=N_SAMPLE, cam_dist=2.0):
    """BASELINE.json's "PSNR vs ref" on the benchmarked frame itself: the HIP path renders the SAME strided sample of the
    512 x 512 frame the CPU leg rendered with the oracle (lib/evaluators/base_evaluator.py:26-29's PSNR on rgb_map).  SURVEY.md:409's
    contract: rgb PSNR >= 50 dB and max |err| <= 1e-2 over every ray whose reference value fp32 itself pins (figures over all rays beside them)."""
    batch, P, stride = sample_batch(H, skin_noise, n_target, cam_dist)
    out = renderer.render(synthetic.to_device(batch, dev))
    torch.cuda.synchronize(dev)
    rgb, rgb_ref = out.rgb_map.float().cpu(), ref.rgb_map.float()
    e = (rgb - rgb_ref).abs()
    mse = float((e ** 2).mean())
    hit, hit_ref = out.acc_map.cpu() > 0, ref.acc_map > 0
    per_ray = e[0].amax(-1)
    bad = ref.get('fp32_unstable', None)
    bad = torch.zeros_like(per_ray, dtype=torch.bool) if bad is None else bad
    mse_s = float((e[0][~bad] ** 2).mean())
    db = lambda m: float('inf') if m == 0 else -10.0 * math.log10(m)
    # schema 3 (round 5): `rgb`, `max_abs`, `rays_over_1e-2` are over ALL sampled rays (as in rounds 1-3); the *_fp32_stable keys beside
    # them leave out the rays the reference's own fp32 arithmetic does not pin (round 4 printed those under the plain names)
    res = {'schema': 3, 'rgb': db(mse), 'max_abs': float(per_ray.max()), 'rays_over_1e-2': int((per_ray > 1e-2).sum()),
           'rgb_fp32_stable': db(mse_s), 'max_abs_fp32_stable': float(per_ray[~bad].max()), 'rays_over_1e-2_fp32_stable': int((per_ray[~bad] > 1e-2).sum()),
           'n_rays': int(rgb.shape[1]), 'fp32_unstable_rays': int(bad.sum()), 'fp32_unstable_source': ref.get('fp32_unstable_source', None),
           'hit_rays': int(hit_ref.sum()), 'hit_mask_agreement': float((hit == hit_ref).float().mean()),
           'sample': f'every {stride}th in-box ray of the benchmarked {H}x{H} frame, skin_noise {skin_noise}',
           'contract': 'SURVEY.md:409: rgb PSNR >= 50 dB and max |err| <= 1e-2, asserted over every ray the reference\'s own fp32 arithmetic pins '
                       '(`*_fp32_stable`; `rgb`, `max_abs`, `rays_over_1e-2` are the same over ALL sampled rays; a ray is fp32-unstable when 3e-7 noise on the traced distances moves its surface point by > 0.1 mm: '
                       'tools/fp32_stability.py, DESIGN.md section 2).  The surface trace runs in compensated arithmetic (config.trace_precision 1).'}
    res['contract_met'] = bool(res['rgb_fp32_stable'] >= 50.0 and res['max_abs_fp32_stable'] <= 1e-2)
    res['contract_met_all_rays'] = bool(res['rgb'] >= 50.0 and res['max_abs'] <= 1e-2)
    # which arithmetic produced these figures: cfg.trace_precision 0 = plain 16-bit operands everywhere, 1 = the surface trace compensated
    # (the shipped default), 2 = every distance query compensated (the tier that meets max <= 1e-2 on EVERY pixel of the full frame and
    # on the hard cases, at 2 x the frame time: tests/test_gpu_parity.py test_full_frame_shadow_tier_is_harmless, test_hard_case_switch_matrix)
    tp = int(renderer.cfg.get('trace_precision', 1))
    res['contract_tier'] = {'trace_precision': tp, 'name': {0: 'plain f16 operands', 1: 'surface trace + shadow rays towards the key lights compensated, the other shadow rays plain f16', 2: 'all distance queries compensated'}[tp],
                            'key_light_share': float(renderer.cfg.get('key_light_share', 0.0))}
    # every sampled ray over 1e-2, by name: its error, whether fp32 itself pins it, and (committed samples) how often the reference's own
    # arithmetic flips it at fp32's noise level (tests/golden/fp32_unstable_rays.json: a coin toss of the reference is not an error of this path)
    over = [int(i) for i in (per_ray > 1e-2).nonzero()[:, 0][:16]]
    if over:
        probs = {}
        src = str(ref.get('fp32_unstable_source', ''))
        if src.startswith('tests/golden/fp32_unstable_rays.json:'):
            d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests', 'golden', 'fp32_unstable_rays.json')))[src.split(':')[1].split(' ')[0]]
            probs = dict(zip(d['unstable'], d.get('flip_probability', {}).get('noise_1.2e-7', [])))
        res['rays_over_1e-2_detail'] = [dict(ray=i, max_abs=float(per_ray[i]), fp32_unstable=bool(bad[i]),
                                             reference_flip_probability_at_fp32_noise=probs.get(i)) for i in over]
    return res


def hbm_traffic_per_launch(kernel, workload='relight512'):
    """HBM bytes per launch of the dominant kernel from the newest committed PMC summary of this command (rocprofv3 --pmc
    FETCH_SIZE / WRITE_SIZE in their own passes, tools/collect_profiles.sh rewrites it whenever kernels change): FETCH_SIZE
    doubled as MI355X_MICROARCH.md prescribes for gfx950 wide reads.  Returns (bytes, file name)."""
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', f'r[0-9][0-9]_{workload}_pmc.csv')))
    for path in reversed(files):
        try:
            total = 0.0
            for kn in kernel.split('+'):           # a launch made of two kernels (the full query): the sum of both
                rows = [l.strip().split(',') for l in open(path) if l.startswith(kn + ',')]
                v = {r[1]: (float(r[2]), int(r[3])) for r in rows}
                total += (2.0 * v['FETCH_SIZE'][0] / v['FETCH_SIZE'][1] + v['WRITE_SIZE'][0] / v['WRITE_SIZE'][1]) * 1024.0
            try:
                rev = subprocess.run(['git', 'log', '-1', '--format=%h', '--', path], capture_output=True, text=True, cwd=os.path.dirname(path)).stdout.strip()
            except Exception:
                rev = ''
            return total, os.path.basename(path) + (f'@{rev}' if rev else '')
        except Exception as ex:
            print(f'bench.py: could not read HBM traffic from {path}: {ex!r}', file=sys.stderr)
            continue
    return None, None


DUMP_BYTES = 64 << 20


def dump_outputs(path, value, name):
    """--dump-outputs: the maps the last timed step returned (a tensor, or a dict of maps [1, rays, C] / [1, rays]) as path/<name>.npy in
    float32.  Beyond DUMP_BYTES in all, every map keeps the same seeded sample of its rays (axis 1), listed in path/sample_rays.npy."""
    import numpy as np
    items = [(name, value)] if isinstance(value, torch.Tensor) else [(k, v) for k, v in value.items() if isinstance(v, torch.Tensor)]
    arrays = {k: v.detach().float().cpu().numpy() for k, v in items}
    if not arrays:
        raise SystemExit('bench.py --dump-outputs: the timed step returned no arrays')
    os.makedirs(path, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES:
        n = {a.shape[1] for a in arrays.values() if a.ndim >= 2}
        if len(n) != 1:
            raise SystemExit(f'bench.py --dump-outputs: {total} bytes of maps without one common ray axis: {[a.shape for a in arrays.values()]}')
        n = n.pop()
        keep = np.sort(np.random.default_rng(0).choice(n, max(1, int(n * DUMP_BYTES / total)), replace=False))
        arrays = {k: a[:, keep] for k, a in arrays.items()}
        np.save(os.path.join(path, 'sample_rays.npy'), keep.astype(np.float64))
    for k, a in arrays.items():
        np.save(os.path.join(path, f'{k}.npy'), np.ascontiguousarray(a))


def launch_ranks(args, argv):
    """parent of an N-rank job: has not initialised the GPU and never does (no exec of a GPU-initialised process either)."""
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + argv
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not lines:
        sys.stdout.write(r.stdout[-4000:])
        raise SystemExit(r.returncode or 1)
    print(lines[-1])
    raise SystemExit(0)


def dry_rank(args, rank, world):
    """the rank program without the HIP engine: process group, shard plan, a stand-in render of this rank's rays, the frame
    all_gather, barrier + MAX reduce, the JSON line.  What the gloo test of the N > 1 path runs.  `--mode novel_light` gathers the
    config-5 payload (3 channels per probe: 24 at 8 probes), `--ground` the full-frame maps of the ground pass (the README command)."""
    dist.init_process_group(args.backend)
    H = args.size
    base = synthetic.make_batch(H, H, seed=0, posed=True)
    P = base.ray_o.shape[1]
    C = 3 * args.probes if args.mode == 'novel_light' else 4
    F = H * H

    def payload(ray_d, near, far, pix):
        """a per-ray (per-pixel with --ground) "image" of C channels that identifies its ray: what a renderer would return"""
        cols = [ray_d[:, 0], ray_d[:, 1], near, far]
        return torch.stack([cols[k % 4] * (1 + k // 4) + (0 if pix is None else pix.float() * 1e-3) for k in range(C)], -1)[None]
    if args.ground:       # full-frame maps: ground pixels carry their index, the human rays are blended in at their pixels
        inds_all = base.mask_at_box.reshape(-1).nonzero()[:, 0]
        ref = torch.zeros(1, F, C)
        ref[0] = torch.arange(F).float()[:, None] * 0.5
        ref[0, inds_all] += payload(base.ray_d[0], base.near[0], base.far[0], None)[0]
    else:
        ref = payload(base.ray_d[0], base.near[0], base.far[0], None)

    def submit(f):
        """frame f: plan, this rank's stand-in render (the payload times a per-frame factor, so that frames cannot be mistaken for one
        another), the frame gather issued without waiting: returns finish() -> gathered frame"""
        pl = shard.make_plan(P, world, base, mask=base.mask_at_box, ground=args.ground, render_chunk_size=65536, use_cache=False)      # per frame, as the timed loop does
        sb = shard.shard_batch(base, rank, world, 65536, pl, args.ground)
        local = payload(sb.ray_d[0], sb.near[0], sb.far[0], None)
        if args.ground:
            pix = sb.get('ground_pix', None)
            pix = torch.arange(F) if pix is None else pix
            g = pix.float()[:, None].expand(-1, C) * 0.5
            g = g.clone()
            inds = sb.ground_inds if 'ground_inds' in sb else base.mask_at_box.reshape(-1).nonzero()[:, 0]
            g[inds] += local[0]
            local = g[None]
        local = local * float(1 + f % 5)
        if world == 1:
            return (lambda: local), pl
        return shard.gather_maps_async(local, P, rank, world, pl, ground=args.ground), pl

    # D frames in flight: the gathers of frames f .. f + D - 1 are outstanding in ONE process group when frame f is collected (what the
    # replica streams of relightableavatar_amd/pipeline.py do on the GPU); every gathered frame must be ITS frame
    D = max(1, args.frames_in_flight)
    good = True

    def run(n, first):
        nonlocal good
        pending, last = [], None

        def collect():
            nonlocal good, last
            g, fin, last = pending.pop(0)
            good = good and torch.equal(fin(), ref * float(1 + g % 5))
        for f in range(first, first + n):
            fin, pl_ = submit(f)
            pending.append((f, fin, pl_))
            if len(pending) == D:
                collect()
        while pending:
            collect()
        return last
    run(args.warmup, 0)
    dist.barrier()
    t0 = time.perf_counter()
    pl = run(args.steps, args.warmup)
    my_ms = (time.perf_counter() - t0) / args.steps * 1e3
    dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    ok = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    seen = torch.ones(1, dtype=torch.float64)
    dist.all_reduce(seen)
    mine = torch.tensor([my_ms, float(pl.counts[rank])], dtype=torch.float64)
    per_rank = [mine.clone() for _ in range(world)]
    dist.all_gather(per_rank, mine)
    if rank == 0:
        dt = float(tt.item())
        g0 = pl.ground if args.ground else pl
        total = g0.F if args.ground else P
        print(json.dumps({'metric': 'rays_per_sec', 'value': H * H * args.steps / dt, 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps,
                          'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3, 'ms_per_step_sequential': dt / args.steps * 1e3,
                          'higher_is_better': True, 'scaling': 'strong',
                          'vs_baseline': None, 'dtype': 'none', 'data': 'dry run: no kernels, plumbing only',
                          'config': {'workload': f'DRY {H}x{H}', 'backend': args.backend, 'gather_ok': bool(ok.item() == 1.0), 'frames_in_flight': D},
                          'ranks_seen': int(seen.item()),
                          'per_rank': {'ms_per_step': [round(float(t[0]), 4) for t in per_rank], 'rays_per_frame': [int(t[1]) for t in per_rank]},
                          'gather': {'collective': f'all_gather_into_tensor ({args.backend}), one per frame, shards padded to the largest',
                                     'bytes_received_per_rank': int(world * g0.n_max * C * 4), 'channels': C,
                                     'pad_fraction': round((world * g0.n_max - total) / max(total, 1), 5)},
                          'roofline': None}))
    dist.destroy_process_group()
    if ok.item() != 1.0:
        raise SystemExit('dry run: the gathered frame differs from the whole frame')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--mode', default='relight', choices=['relight', 'sphere_tracing', 'anisdf', 'novel_light'])
    ap.add_argument('--probes', type=int, default=8, help='novel_light: number of 16x32 probes re-shaded per frame')
    ap.add_argument('--dtype', default='f16', choices=['f16', 'bf16'])
    ap.add_argument('--full', action='store_true', help='also run the legs beside the headline figure: CPU baseline + PSNR vs the oracle, the strictly sequential frames, the pre-posed comparison of --animate')
    ap.add_argument('--dump-outputs', default='', metavar='DIR', help='rank 0 writes the maps the last timed step returned to DIR/<name>.npy (float32; at most 64 MB in all, a seeded sample of rays beyond that)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--ground', action='store_true', help='relight: add the ground-plane pass (cfg.vis_ground_shading, SURVEY.md 8f row N1)')
    ap.add_argument('--emulate-world', type=int, default=0, help='tuning aid: render only rank 0\'s shard of an N-rank job on one GPU (no collective); value is then NOT a whole-job rate')
    ap.add_argument('--emulate-rank', type=int, default=0, help='with --emulate-world: which rank\'s shard to render (load balance of the tile deal)')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'], help='nccl == RCCL on ROCm; gloo only with --dry')
    ap.add_argument('--share-gpu', action='store_true', help='with --backend gloo: the REAL rank program (HIP engine, shard plan, frames in flight) as N processes that all render on GPU 0, the frame gather staged through pinned host memory over gloo (RCCL refuses two ranks on one device): the multi-process test of the N > 1 path on a 1-GPU box; not a performance mode')
    ap.add_argument('--dump-frame', default='', help='rank 0 writes the last timed frame (the gathered maps, channels concatenated) to this .npy file')
    ap.add_argument('--dry', action='store_true', help='no HIP engine: launcher + process-group plumbing on CPU tensors (CPU test of the N > 1 path)')
    ap.add_argument('--static-frame', action='store_true', help='A/B: do not re-pose the body every step (round-1 behaviour: per-frame set-up outside the timed region)')
    ap.add_argument('--k4-batch', type=int, default=0, help='cfg.k4_batch_slots: full queries per forward+backward launch pair (0 = library default)')
    ap.add_argument('--soak', type=float, default=3.0, help='seconds of untimed frames BEFORE the W warm-up steps: the chip is power-limited on this path (DESIGN.md section 4), so the clock of a cold 0.7 s burst is not the sustained one')
    ap.add_argument('--frames-in-flight', type=int, default=3, help='frames kept in flight on as many HIP streams (relightableavatar_amd/pipeline.py): the latency-bound small-kernel phase of frame f + 1 runs beside the light-visibility stage of frame f, the stages themselves are serialised by a gate.  1 = strictly sequential frames')
    ap.add_argument('--animate', action='store_true', help='every step renders a DIFFERENT frame of an animation: bone poses -> body state on the device (N3, ra_pose_frame) -> rays + box culling on the device (N2, ra_gen_rays) -> set_frame -> render, all inside the timed region and all asynchronous (the rays of a frame are generated one pipeline turn ahead; their count is read back behind an event)')
    ap.add_argument('--coverage', type=float, default=0.0, help='fraction of the frame the body covers: moves the camera in (0 = SURVEY.md 8d camera at 2 m, ~8 %% hit pixels; 0.35 = a frame-filling subject, camera at 0.96 m)')
    ap.add_argument('--no-sequential', action='store_true', help='with --full: skip the strictly sequential leg (ms_per_step_sequential: one frame at a time, host sync after each, as the reference loop run.py:43-49)')
    ap.add_argument('--trace-precision', type=int, default=1, choices=[0, 1, 2], help='cfg.trace_precision: 1 = the surface trace in compensated arithmetic (default), 0 = plain 16-bit operands everywhere (round 3), 2 = compensated everywhere')
    ap.add_argument('--body', default='blob', choices=['blob', 'split'], help='split: the hard-case body of tests/golden/switches.npz `split_body` (synthetic.SPLIT_BODY_KW: a horn pulled 0.57 m out of the body, shadowing it at distance) under the front key light, 12 shadow iterations unless --shadow-iters says otherwise')
    ap.add_argument('--weights', default='init', choices=['init', 'sharp'], help='sharp: trained-like synthetic weights (synthetic.SHARP_BANDS: live high-frequency encoding columns, cm-scale surface detail)')
    ap.add_argument('--shadow-iters', type=int, default=0, help='cfg.obj_lvis.iter (0 = the reference default 4; --body split: 12)')
    ap.add_argument('--key-light-share', type=float, default=-1.0, help='cfg.key_light_share (default: the configuration default 0.0078; 0 = no key-light tier: every shadow ray on plain f16 operands, round 5)')
    ap.add_argument('--skin-noise', type=float, default=2.0, help='synthetic body: per-vertex noise of the skinning logits (SURVEY.md 8d default 2.0; 0 = smooth, SMPL-like)')
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit('bench.py: --steps must be at least 1')

    if args.gpus > 1 and 'RANK' not in os.environ:
        launch_ranks(args, sys.argv[1:])
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local = int(os.environ.get('LOCAL_RANK', 0))
    if world != max(args.gpus, 1) and 'RANK' in os.environ and args.gpus != 1:
        raise SystemExit(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world}')
    if args.dry:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if 'RANK' not in os.environ:
            os.environ.setdefault('MASTER_PORT', '29577')
            os.environ.update(RANK='0', WORLD_SIZE='1')
        return dry_rank(args, rank, world)
    if args.backend != 'nccl' and not args.share_gpu:
        raise SystemExit('bench.py: the render path runs on MI355X GPUs over RCCL (backend nccl); gloo is for --dry and --share-gpu')
    if args.share_gpu and args.backend != 'gloo':
        raise SystemExit('bench.py --share-gpu: N ranks on one device need --backend gloo (RCCL refuses two ranks on a device)')
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs MI355X GPUs (the render path has no CPU fallback)')
    local = 0 if args.share_gpu else local
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    use_dist = world > 1 or 'RANK' in os.environ       # under torchrun the RCCL path runs even at world size 1
    sdev = torch.device('cpu') if args.share_gpu else dev          # where the job's statistics are reduced (gloo moves host tensors)
    if use_dist:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if args.share_gpu:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=dev)

    H = args.size
    kw = dict(vis_ground_shading=True, ground_normal=[0.0, -1.0, 0.0], ground_origin=[0.0, 0.45, 0.0]) if args.ground else {}
    if args.k4_batch:
        kw['k4_batch_slots'] = args.k4_batch
    if args.mode == 'novel_light':
        kw['novel_light_timing'] = False     # nobody reads `diff` here: no host sync inside the frame
    kw['trace_precision'] = args.trace_precision
    if args.key_light_share >= 0:
        kw['key_light_share'] = args.key_light_share
    cfg = make_cfg(args.mode, mlp_dtype=args.dtype, **kw)
    if args.body == 'split':
        BODY_KW.update(synthetic.SPLIT_BODY_KW)
        WEIGHTS_KW['env'] = 'front'
    if args.weights != 'init':
        WEIGHTS_KW['kind'] = args.weights
    shadow_iters = args.shadow_iters or (12 if args.body == 'split' else 0)
    if shadow_iters and 'obj_lvis' in cfg:
        cfg.obj_lvis.iter = shadow_iters
    relight = args.mode in ('relight', 'novel_light')
    D = max(1, args.frames_in_flight)
    pipe = FramePipeline(cfg, synthetic.make_state_dict(0, relight=relight, cfg=cfg, **WEIGHTS_KW), dev, depth=D)
    net, renderer = pipe.networks[0], pipe.renderers[0]
    # one batch per replica: a frame in flight owns its body state and its in-place grown box until it has been consumed
    cam_dist = cam_dist_of(args.coverage)
    bases = [synthetic.to_device(synthetic.make_batch(H, H, seed=0, posed=True, n_novel_lights=args.probes if args.mode == 'novel_light' else 0,
                                                      skin_noise=args.skin_noise, cam_dist=cam_dist, **BODY_KW), dev) for _ in range(D)]
    base = bases[0]
    P = base.ray_o.shape[1]
    wb0 = base.wbounds.clone()
    mask0 = base.mask_at_box.clone()
    engs = pipe.engines()

    mask_host = base.mask_at_box.cpu()          # the loader's copy: the shard plan is host work (shard.make_plan)
    wbh0 = wb0.cpu()
    nw = args.emulate_world if args.emulate_world > 1 else world          # --emulate-world N: rank 0's share of an N-rank job, no collective
    rk = args.emulate_rank if args.emulate_world > 1 else rank

    frame_no = [0]

    def frame(net_r, rend_r):
        base = bases[frame_no[0] % D]
        eng = net_r.engine()
        # a fresh batch per frame, as the reference's loader delivers: body box (device tensor + the loader's host copy), mask
        base.wbounds.copy_(wb0)
        base.wbounds_host, base.wbounds_host_version = wbh0.clone(), base.wbounds._version
        if not args.static_frame:
            eng.set_frame(base, force=True)     # an animation poses a new body every frame: vertex blend, BVH build, bias folds are timed
        if args.ground:
            base.mask_at_box.copy_(mask0)   # the ground pass sets it to all-true in place (sphere_tracing_renderer.py:1103)
        # a new frame has a new mask: the shard plan (ownership + exchange index vectors) is rebuilt every step, inside the timed region
        pl = shard.make_plan(P, nw, base, dev, mask=mask_host, ground=args.ground, render_chunk_size=cfg.render_chunk_size, use_cache=False) if nw > 1 else None
        if args.mode == 'novel_light':      # config 5: main pass + all probes re-shaded in one launch (per-rank shard)
            out = rend_r.render(shard.shard_batch(base, rk, nw, cfg.render_chunk_size, pl, args.ground))
            rgb = torch.cat([out[n].rgb_map for n in base.novel_lights], dim=-1)
            return rgb if args.emulate_world > 1 else shard.gather_maps(rgb, P, rank, world, plan=pl, ground=args.ground)
        if args.emulate_world > 1:
            return rend_r.render(shard.shard_batch(base, rk, nw, cfg.render_chunk_size, pl, args.ground))
        return shard.render_sharded(rend_r, base, ('rgb_map', 'acc_map'), rank, world, plan=pl)

    anim = None
    if args.animate:
        import numpy as np
        if args.mode not in ('relight', 'sphere_tracing') or args.ground:
            raise SystemExit('bench.py --animate: relight / sphere_tracing without the ground pass')
        sk = synthetic.make_skeleton(0)
        e0 = engs[0]
        Tn = torch.from_numpy
        tv_d, w_d = Tn(sk.tverts).to(dev), Tn(sk.weights).to(dev)
        eye = np.tile(np.eye(4, dtype=np.float32), (sk.poses.shape[0], 1, 1))
        zero3 = np.zeros(3, np.float32)
        # the big-pose bone transforms: the same device routine posed with the big pose
        big_A = e0.pose_frame(sk.big_poses, sk.tjoints, sk.parents, tv_d, w_d, eye, sk.faces, zero3, zero3).A.cpu().numpy()
        n_anim = 48
        ph = np.arange(sk.poses.size, dtype=np.float32).reshape(sk.poses.shape)
        seq = [dict(poses=(sk.poses + 0.06 * np.sin(0.37 * f + ph)).astype(np.float32),
                    Rh=(sk.Rh + np.array([0.0, 0.05 * np.sin(0.21 * f), 0.0], np.float32)).astype(np.float32),
                    Th=(sk.Th + np.array([0.01 * np.sin(0.3 * f), 0.0, 0.01 * np.cos(0.3 * f)], np.float32)).astype(np.float32)) for f in range(n_anim)]
        Kc, Rc, Tc = synthetic.make_camera(H, H, origin=(0.0, 0.0, -cam_dist))
        from relightableavatar_amd.data_utils import DeviceFrameLoader
        loader = DeviceFrameLoader(H, H, Kc, Rc, Tc, sk.tjoints, sk.parents, tv_d, w_d, big_A, sk.faces, mask_to_host=nw > 1)
        anim = dotdict(ahead=[None] * D, wait=0.0, rays=0, cached=None)

        def issue(eng, f):
            """N3 + N2 of animation frame f on the current stream: body state, then the rays against its box — nothing waits"""
            q = seq[f % n_anim]
            return loader.issue(eng, q['poses'], q['Rh'], q['Th'])

        def frame_animate(net_r, rend_r):
            f = frame_no[0]
            r = pipe.networks.index(net_r)       # the replica this frame runs on: its stream carries the frame issued ahead for it
            eng = net_r.engine()
            if anim.cached is not None:          # the comparison leg: the same frames, posed and culled BEFORE the loop (a loader that is never the bottleneck)
                b = dotdict(anim.cached[f % n_anim])
                b.wbounds = b.wbounds.clone()    # the renderer grows the box in place
                b.wbounds_host, b.wbounds_host_version = b.wbounds_host.clone(), b.wbounds._version
                if args.emulate_world > 1 or nw > 1:
                    raise SystemExit('bench.py --animate: the pre-posed comparison leg is single-GPU')
                return shard.render_sharded(rend_r, b, ('rgb_map', 'acc_map'), rank, world, plan=None)
            pend = anim.ahead[r] or issue(eng, f)
            t_w = time.perf_counter()
            b = loader.batch(pend)               # an event: the kernels that made these rays were queued a pipeline turn ago
            anim.wait += time.perf_counter() - t_w
            P_f = b.ray_o.shape[1]
            anim.rays += P_f
            pl = shard.make_plan(P_f, nw, b, dev, mask=b.get('mask_host', None), render_chunk_size=cfg.render_chunk_size, use_cache=False) if nw > 1 else None
            if args.emulate_world > 1:
                out = rend_r.render(shard.shard_batch(b, rk, nw, cfg.render_chunk_size, pl))
            else:
                out = shard.render_sharded(rend_r, b, ('rgb_map', 'acc_map'), rank, world, plan=pl)
            anim.ahead[r] = issue(eng, f + D)    # this replica's next frame: posed and culled behind this one, read a turn later
            return out

    def step():
        if anim is not None:
            p = pipe.submit(fn=frame_animate)
            frame_no[0] += 1
            return p
        # queued on the next replica's stream (frames-in-flight 1: the current stream); the timed region ends with a device-wide sync
        p = pipe.submit(fn=frame)
        frame_no[0] += 1
        return p

    def sync():
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize(dev)

    # sustained clocks / temperature before anything is measured: rank 0 sizes the soak from two probe frames, every rank runs the
    # same number of frames (the frame all_gather is a collective)
    n_soak = 0
    if args.soak > 0:
        step(); step(); sync()                  # cold frames (allocations, first launches): not a measure of anything
        t_probe = time.perf_counter()
        for _ in range(3):
            step()
        sync()
        ns = torch.tensor([max(0, int(args.soak / max((time.perf_counter() - t_probe) / 3, 1e-4)))], device=sdev)
        if use_dist:
            dist.broadcast(ns, 0)
        n_soak = int(ns.item())
        if anim is not None:      # the timed steps start at frame 0 of the pose cycle whatever the soak measured: the same inputs every run
            n_soak += -(5 + n_soak + args.warmup) % n_anim
        for _ in range(n_soak):
            step()
        n_soak += 5
    for _ in range(args.warmup):
        step()
    sync()
    for e in engs:
        e.reset_counters()
        e.enable_timing(True)
    sync()
    frame_start = frame_no[0]
    if anim is not None:
        anim.wait, anim.rays = 0.0, 0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    t_host = time.perf_counter() - t0           # all steps queued: the host's share (the GPU is the bound while this stays below dt)
    sync()
    dt = time.perf_counter() - t0
    t_wait = anim.wait if anim is not None else 0.0
    for e in engs:
        e.enable_timing(False)
    if args.dump_frame and rank == 0:          # the last timed frame as the job assembled it (the multi-process test compares it bit for bit)
        import numpy as np
        v = out.result()
        v = v if isinstance(v, torch.Tensor) else torch.cat([v[k] if v[k].ndim == 3 else v[k][..., None] for k in ('rgb_map', 'acc_map')], dim=-1)
        torch.cuda.synchronize(dev)
        np.save(args.dump_frame, v.float().cpu().numpy())
    # the strictly sequential loop beside it: one frame at a time, the host waits for each (the reference's loop, run.py:43-49) — this is
    # also a frame's first-to-last-launch latency.  Counters / kernel timers are off: the roofline figures are the timed region's.
    dt_seq = None
    cnt_snapshot = [dict(e.counters()) for e in engs]
    if args.dump_outputs and rank == 0:         # what the last timed step returned (after the snapshot: reading lazy maps launches work)
        dump_outputs(args.dump_outputs, out.result(), 'rgb_probes' if args.mode == 'novel_light' else 'out')
        torch.cuda.synchronize(dev)
    if args.full and not args.no_sequential:
        n_seq = max(2, min(args.steps, 10))
        sync()
        t1 = time.perf_counter()
        for _ in range(n_seq):
            step()
            torch.cuda.synchronize(dev)
        sync()
        dt_seq = (time.perf_counter() - t1) / n_seq
    dt_static = None
    if anim is not None:
        rays_per_frame_anim = anim.rays / max(args.steps, 1)
    if args.full and anim is not None and nw == 1:          # the same frames through the same pipeline with N3 + N2 done BEFORE the loop: what posing / culling inside it costs
        sync()
        anim.cached = [loader.batch(issue(e0, f)) for f in range(n_anim)]
        sync()
        frame_no[0] = 0
        for _ in range(D + 2):
            step()
        sync()
        frame_no[0] = frame_start % n_anim          # the same stretch of the pose cycle as the timed region
        t2 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        dt_static = (time.perf_counter() - t2) / args.steps
    my_ms = dt / args.steps * 1e3
    tt = torch.tensor([dt, dt_seq or 0.0], device=sdev, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt, dt_seq = float(tt[0].item()), (float(tt[1].item()) if dt_seq is not None else None)
    cnt = dotdict()
    for c_e in cnt_snapshot:                        # every replica counted its own frames (snapshot taken before the sequential leg)
        for k, v in c_e.items():
            cnt[k] = cnt.get(k, 0) + v
    # the dominant kernel: the full query on the volume path, else the 8-wave distance query (the launches that fill the chip; kind 2) —
    # a frame without such launches (sphere tracing at 512 x 512, a small rank share) reports all distance-query launches (kind 0)
    wide = args.mode != 'anisdf' and cnt.get('n_fine_sdf_wide', 0) > 0
    # ... and a sphere-tracing frame whose distance queries all ran in the compensated tier reports that kernel (kind 4)
    comp_only = args.mode != 'anisdf' and not wide and cnt.get('n_fine_sdf_comp', 0) > 0 and cnt.get('n_fine_sdf_comp', 0) >= 0.9 * cnt.get('n_fine_sdf', 0)
    kind = 1 if args.mode == 'anisdf' else (2 if wide else (4 if comp_only else 0))
    mlp_ms, mlp_launches = 0.0, 0
    for e in engs:
        ms_e, n_e = e.kernel_time(kind)
        mlp_ms, mlp_launches = mlp_ms + ms_e, mlp_launches + n_e
    cnts = torch.tensor([cnt.n_fine_sdf, cnt.n_fine_full, cnt.n_coarse, cnt.n_hit_pixels, cnt.n_shadow_rays], device=sdev, dtype=torch.float64)
    # what makes the driver's SCALE record checkable: how many ranks really took part, and every rank's own time and share of the work
    seen = torch.ones(1, device=sdev, dtype=torch.float64)
    mine = torch.tensor([my_ms, cnt.n_hit_pixels / max(args.steps, 1), cnt.n_fine_sdf / max(args.steps, 1)], device=sdev, dtype=torch.float64)
    per_rank = [mine.clone() for _ in range(world)]
    if use_dist:
        dist.all_reduce(cnts)
        dist.all_reduce(seen)
        dist.all_gather(per_rank, mine)
    if rank == 0:
        ms = dt / args.steps * 1e3
        kname = 'mlp_sdf_stream_kernel<f16|bf16, 8>' if wide else ('mlp_sdf_comp_kernel (compensated: 3 MFMAs per algorithmic one)' if comp_only else 'mlp_sdf_stream_kernel')
        units, f_unit = (cnt.n_fine_sdf_wide if wide else (cnt.n_fine_sdf_comp if comp_only else cnt.n_fine_sdf)), F_SDF
        if args.mode == 'anisdf':           # the volume path has no distance-only queries: its dominant kernel is the full query
            # the full query = two kernels per launch (forward with tape, reverse-mode backward + colour net); the timer brackets both
            kname, units, f_unit = 'mlp_fwd_tape_kernel+mlp_bwd_heads_kernel', cnt.n_fine_full, F_FULL_ANISDF
        achieved = (units * f_unit) / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else 0.0
        default_cmd = args.mode == 'relight' and H == 512 and world == 1 and wide and not args.ground and args.emulate_world <= 1
        traffic, traffic_src = hbm_traffic_per_launch('mlp_sdf_stream_kernel_w8') if default_cmd else (None, None)
        if args.mode == 'anisdf' and H == 512 and world == 1 and '+' in kname:
            # the PMC summary is per DISPATCH; one timed launch (a full-query call) is ceil(samples / k4 batch) dispatch pairs
            traffic, traffic_src = hbm_traffic_per_launch(kname, 'anisdf512')
            chunk_rays = min(P, max(int(cfg.render_chunk_size), int(cfg.get('volume_chunk_rays', 65536))))
            pairs = -(-chunk_rays * int(cfg.n_samples) // (args.k4_batch or (1 << 20)))
            traffic = None if traffic is None else traffic * pairs
        line = {
            'metric': 'rays_per_sec', 'value': H * H * args.steps / dt, 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
            'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': f'xuzhen_12v_geo_fix_mat-shaped full relight, {H}x{H}, 16x32 light probe, DFSS visibility ({int(cfg.obj_lvis.iter) if "obj_lvis" in cfg else 4} iters), '
                                   f'16-iter surface trace, synthetic weights/body' + (f', {args.probes} novel probes re-shaded' if args.mode == 'novel_light' else '') + (', + ground-plane pass' if args.ground else '') if relight else f'{args.mode} {H}x{H}',
                       'rays_per_frame': H * H, 'rays_in_bbox': P, 'hit_pixels_per_frame': int(cnts[3].item() / args.steps),
                       'fine_queries_per_frame': int(cnts[0].item() / args.steps), 'full_queries_per_frame': int(cnts[1].item() / args.steps),
                       'coarse_queries_per_frame': int(cnts[2].item() / args.steps),
                       'shadow_rays_per_frame': int(cnts[4].item() / args.steps),
                       'parallelism': f'8x8 pixel tiles dealt over {world} ' + ('rank processes SHARING GPU 0 (multi-process test mode, not a rate)' if args.share_gpu else 'GPU(s)') + ' + one all_gather'},
            'roofline': {'bound': 'mfma', 'achieved': achieved, 'peak': MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / MFMA_PEAK_TFLOPS,
                         'traffic': traffic, 'traffic_source': 'offline' if traffic is not None else None,
                         'traffic_unit': f'B/launch; NOT measured in this run: rocprofv3 --pmc passes of this command (FETCH_SIZE x 2 + WRITE_SIZE), profiles/{traffic_src}',
                         'kernel': kname, 'launches': mlp_launches,
                         'avg_launch_ms': mlp_ms / max(mlp_launches, 1), 'flop_per_unit': f_unit,
                         'units_per_launch': units / max(mlp_launches, 1)},
        }
        line['ms_per_step_sequential'] = None if dt_seq is None else dt_seq * 1e3       # one frame at a time, host sync after each: the reference's loop, and a frame's latency
        line['ranks_seen'] = int(seen.item())
        line['per_rank'] = {'ms_per_step': [round(float(t[0]), 4) for t in per_rank], 'hit_pixels_per_frame': [int(t[1]) for t in per_rank],
                            'fine_queries_per_frame': [int(t[2]) for t in per_rank]}
        if world > 1 and not args.emulate_world > 1:
            C_g = 3 * args.probes if args.mode == 'novel_light' else 4
            pl0 = shard.make_plan(P, world, base, dev, mask=mask_host, ground=args.ground, render_chunk_size=cfg.render_chunk_size, use_cache=False)
            g0 = pl0.ground if args.ground else pl0
            total = g0.F if args.ground else P
            line['gather'] = {'collective': f'all_gather_into_tensor ({"gloo, staged through pinned host memory: N ranks on ONE GPU" if args.share_gpu else "RCCL"}), one per frame, shards padded to the largest',
                              'bytes_received_per_rank': int(world * g0.n_max * C_g * 4), 'channels': C_g,
                              'pad_fraction': round((world * g0.n_max - total) / max(total, 1), 5)}
        line['hit_pixels_per_sec'] = cnts[3].item() / dt          # the 84 % of rays that miss the box cost nothing: rays/s flatters
        line['fine_queries_per_sec'] = cnts[0].item() / dt
        line['config']['frame_setup'] = 'static frame (set-up excluded)' if args.static_frame else 'per-frame body state (vertex blend, BVH build, bias folds) re-run every step inside the timed region'
        line['config']['soak'] = f'{n_soak} untimed frames (about {args.soak:.1f} s, sized from three probe frames after two cold ones) before the {args.warmup} warm-up steps'
        line['config']['soak_frames'] = n_soak
        line['config']['frames_in_flight'] = D
        line['config']['camera_distance_m'] = round(cam_dist, 4)
        line['config']['trace_precision'] = args.trace_precision
        line['config']['key_light_share'] = float(cfg.get('key_light_share', 0.0))
        line['config']['k3cc_enabled'] = bool(engs[0].k3cc_enabled())
        line['config']['body'], line['config']['weights'], line['config']['shadow_iters'] = args.body, args.weights, int(cfg.obj_lvis.iter) if 'obj_lvis' in cfg else None
        line['config']['fine_queries_compensated_per_frame'] = int(cnt.get('n_fine_sdf_comp', 0) / args.steps)
        if args.emulate_world > 1:
            line['config']['emulate_world'], line['config']['emulate_rank'] = args.emulate_world, args.emulate_rank
        line['host_enqueue_ms_per_step'] = (t_host - t_wait) / args.steps * 1e3
        if anim is not None:
            line['host_wait_ms_per_step'] = t_wait / args.steps * 1e3         # back-pressure: waiting for the count of rays generated one pipeline turn earlier
            line['config']['animate'] = (f'{n_anim}-frame pose cycle: per step ra_pose_frame (N3: bone transforms, LBS, normals, bounds on the device) + '
                                         f'ra_gen_rays against the new box (N2) + set_frame + render; rays of frame f generated {D} steps ahead')
            line['config']['rays_in_bbox'] = int(rays_per_frame_anim)
            if dt_static is not None:
                line['ms_per_step_frames_posed_before_the_loop'] = dt_static * 1e3          # the same frames, N3 + N2 outside the loop
                line['animate_over_preposed'] = dt / args.steps / dt_static
        if args.full and world == 1 and not args.no_cpu_baseline:
            line['cpu_baseline'], ref = cpu_baseline(cfg, H, args.skin_noise, cam_dist=cam_dist)
            if args.mode in ('relight', 'sphere_tracing', 'anisdf') and not args.ground and args.emulate_world <= 1:
                try:
                    line['psnr_vs_oracle'] = psnr_vs_oracle(renderer, ref, H, args.skin_noise, dev, cam_dist=cam_dist)
                except Exception as ex:             # a line without its parity figure is not a result
                    print(json.dumps(line))
                    raise SystemExit(f'bench.py: psnr_vs_oracle could not be computed: {ex!r}')
        print(json.dumps(line))
    if use_dist:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

"""One optimisation step of fitting.fit_heads (loss, backward) on the hit pixels of a 512 x 512 relit frame: the material heads through
ra_heads_forward / ra_heads_backward against the same step with the heads evaluated by torch (F.linear, fp32, autograd) on the same
device.  Appends one JSON line to profiles/heads_train.jsonl.  A record, not a gate: there is no pass threshold.

    python tools/bench_heads.py [--out profiles/heads_train.jsonl] [--size 512] [--reps 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_heads.py --out /dev/null --reps 5 --kernels-only      # a run of its own
    python tools/bench_heads.py --share DIR [--out ...]      # the heads kernels' share of that trace's kernel time, appended as a line
    python tools/bench_heads.py --regularisers [--out profiles/relight_reg.jsonl]      # the regularised step (fit_heads(regularisers=True))
    python tools/bench_heads.py --light-noise [--out profiles/light_noise.jsonl]       # ... under the trainer's light-position noise

--regularisers times, on the same frame: the step without regularisers (the figure above, `kernels`), the step of the trainer's loss with
ra_canonical_features / ra_gaussian_entropy, and that step with the two entropy terms evaluated by torch (the reference's formulas under
autograd on the same device tensors); and ra_canonical_features against ra_bigpose_features on the frame's samples.

--light-noise times the regularised step of fit_heads on the same frame for three settings — light_noise off, on with all counted pixels,
on with pixels_per_step = 1024 — and, for scale, one Engine.light_visibility call on all counted pixels and one render of the frame.
Under rocprofv3 (a run of its own, a few --reps, --out /dev/null) --share DIR then names the kernels the added time goes to (`top`).

Both variants are warmed up (code objects, ctx scratch, clocks), then timed interleaved with HIP events around a whole step; the median
and the spread are reported.  Everything but the heads is shared: the composite in torch, ra_reshade and ra_reshade_backward.
A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

HEADS_KERNELS = ('heads_kernel', 'heads_dw_kernel', 'heads_slab_sum_kernel', 'heads_pack_kernel', 'heads_absmax_kernel')


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def torch_heads(eng, theta, feat):
    """the two heads on the flat parameters in fp32 under autograd (what a torch port of the trainer would run)"""
    cfg = eng.cfg
    shapes = [(128, 256), (128,), (128, 128), (128,), (3, 128), (3,), (128, 256), (128,), (128, 128), (128,), (1, 128), (1,)]
    t, o = [], 0
    for sh in shapes:
        n = int(torch.Size(sh).numel())
        t.append(theta[o:o + n].reshape(sh))
        o += n

    def run(q, slope, bias):
        x = feat
        for i in range(3):
            x = F.linear(x, q[2 * i], q[2 * i + 1])
            if i < 2:
                x = F.softplus(x, beta=100)
        return slope * torch.sigmoid(x) + bias
    return run(t[:6], cfg.albedo_slope, cfg.albedo_bias), run(t[6:], cfg.roughness_slope, cfg.roughness_bias)[:, 0]


def torch_entropy(eng, x, bins=15):
    """lib/utils/loss_utils.py:51-76 as a torch port would run it (fp32 autograd on the device)"""
    x = x.reshape(-1, 3)
    sigma = x.var(dim=0)
    centers = (torch.arange(bins, device=x.device, dtype=x.dtype) + 0.5) / bins
    k = (-0.5 * ((x[None] - centers[:, None, None]) / sigma).pow(2)).exp() / (sigma * 2.5066282746310002) / bins
    h = k.sum(dim=1)
    e = 0
    for i in range(3):
        hi = h[:, i]
        hi = hi / hi.sum() + 1e-6 if hi.sum() > 1e-6 else torch.ones_like(hi)
        e = e + torch.sum(-hi * torch.log(hi))
    return e


def timed(variants, reps, warm=3):
    """{name: [ms]}: the variants warmed up, then timed interleaved with HIP events around a whole call"""
    for _ in range(warm):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, f in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1))
    return t


def regularised_leg(args, eng, cfg, cache, theta, probe, fitting):
    dev = eng.device
    c = cache[0]
    n = c.cpts.shape[0]
    weights = fitting.regulariser_weights(cfg, True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    noise = lambda: [torch.normal(0.0, float(cfg.xyz_noise_std), (n, 3), generator=gen, device=dev)]

    def step(**ops):
        theta.grad = None
        fitting.regularised_loss(eng, cache, theta, probe, weights, noise(), **ops)[0].backward()

    def plain():
        theta.grad = None
        fitting.heads_loss(eng, cache, theta, probe).backward()
    t = timed([('plain', plain)], args.reps)          # on its own, as the default leg times it: the figure to hold against the parent commit's
    t.update(timed([('regularised', step), ('regularised_torch_entropy', lambda: step(entropy=torch_entropy))], args.reps))
    bpts, cpts, out = torch.rand(n, 3, device=dev) * 0.2 + 0.3, c.cpts, torch.empty(n, 256, device=dev)
    t.update(timed([('bigpose_features', lambda: eng.bigpose_features(bpts)), ('canonical_features', lambda: eng.canonical_features(cpts, out=out)),
                    ('gaussian_entropy', lambda: eng.gaussian_entropy(cpts))], args.reps))
    r = dict(tool='bench_heads', kind='regularised_step', size=args.size, hit_pixels=int(c.w.shape[0]), samples=n, reps=args.reps,
             device=torch.cuda.get_device_name(0), weights=weights)
    for k, v in t.items():
        r[k + '_ms'] = round(median(v), 4)
        r[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
    r['regularised_over_plain'] = round(r['regularised_ms'] / r['plain_ms'], 3)
    r['canonical_over_bigpose'] = round(r['canonical_features_ms'] / r['bigpose_features_ms'], 3)
    r['note'] = ('one loss + backward of fit_heads without the Adam update; plain: the image loss alone; regularised: the trainer\'s loss with fresh '
                 'device noise per step; *_torch_entropy: the two entropy terms by torch autograd instead of ra_gaussian_entropy; the three last '
                 'figures are single calls on the frame\'s samples (host launch overhead included)')
    return r


def light_noise_leg(args, eng, cfg, net, batch, maps, theta, probe, fitting, render):
    dev = eng.device
    weights = fitting.regulariser_weights(cfg, True)
    target = maps.rgb_map.reshape(-1, 3) * 0.9
    with torch.no_grad():
        still = fitting._frame_cache(eng, cfg, batch, maps, target, None, True)
        moving = fitting._frame_cache(eng, cfg, batch, maps, target, None, True, retrace=True)
    n, S = still.w.shape[0], still.S
    xyz0 = fitting.loaded_light_xyz(net, cfg, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    normal = lambda std, rows: torch.normal(0.0, float(std), (rows, 3), generator=gen, device=dev)

    def step(c, noisy, pixels):
        theta.grad = None
        xyz = xyz0 + normal(cfg.light_xyz_noise_std, xyz0.shape[0]) if noisy else None
        rows = torch.randperm(n, generator=gen, device=dev)[:pixels] if pixels else None
        v, shade = fitting.step_frame(eng, c, probe, rows, xyz)
        fitting.regularised_loss(eng, [v], theta, probe, weights, [normal(cfg.xyz_noise_std, v.cpts.shape[0])], shades=[shade])[0].backward()
    sub = min(1024, n)
    t = timed([('off', lambda: step(still, False, None)), ('on_all_pixels', lambda: step(moving, True, None)),
               (f'on_{sub}_pixels', lambda: step(moving, True, sub)), (f'off_{sub}_pixels', lambda: step(still, False, sub))], args.reps)
    if not args.kernels_only:
        t.update(timed([('light_visibility_all_pixels', lambda: eng.light_visibility(moving.surf_pts, moving.norm_pts, moving.acc, moving.bbox, probe=probe)),
                        ('render_frame', render)], max(3, args.reps // 4)))
    eng.set_frame(batch)
    r = dict(tool='bench_heads', kind='light_noise_step', size=args.size, hit_pixels=int(n), samples=int(n * S), lights=int(xyz0.shape[0]), reps=args.reps,
             device=torch.cuda.get_device_name(0), light_xyz_noise_std=float(cfg.light_xyz_noise_std), weights=weights)
    for k, v in t.items():
        r[k + '_ms'] = round(median(v), 4)
        r[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
    r['on_all_over_off'] = round(r['on_all_pixels_ms'] / r['off_ms'], 3)
    r[f'on_{sub}_over_off'] = round(r[f'on_{sub}_pixels_ms'] / r['off_ms'], 3)
    r['note'] = ('one regularised loss + backward of fit_heads without the Adam update, fresh device noise per step; off: the cached visibility; '
                 'on_*: lights moved and the visibility of the step\'s pixels traced again (Engine.light_visibility); light_visibility_all_pixels: that '
                 'call alone; render_frame: one render of the frame (all stages, every probe of the batch); host launch overhead included')
    return r


def share(trace_dir):
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not files:      # a rocpd database (rocprofv3's default output format): summarised by tools/rocpd_stats.py
        dbs = glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True)
        assert dbs, f'no *kernel_stats.csv and no *_results.db under {trace_dir}'
        import rocpd_stats
        files = [dbs[0][:-len('_results.db')] + '_kernel_stats.csv']
        rocpd_stats.main(dbs[0], files[0])
    total, heads, rows = 0.0, 0.0, {}
    for row in csv.DictReader(open(files[0])):
        ns = float(row.get('TotalDurationNs') or row.get('TotalDuration(ns)') or 0)
        name = row.get('Name') or row.get('KernelName') or ''
        total += ns
        for k in HEADS_KERNELS:
            if k in name:
                heads += ns
                rows[k] = rows.get(k, 0.0) + ns
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = (row.get('Name') or row.get('KernelName') or '').replace('(anonymous namespace)::', '')
        name = (name[5:] if name.startswith('void ') else name).split('(')[0].split('<')[0] or name      # the kernel's name without return type, template and argument lists
        per[name] = per.get(name, 0.0) + float(row.get('TotalDurationNs') or row.get('TotalDuration(ns)') or 0)
    top = [dict(kernel=k[:60], ms=round(v / 1e6, 3), share=round(v / total, 4)) for k, v in sorted(per.items(), key=lambda kv: -kv[1])[:8]] if total else []
    return dict(tool='bench_heads', kind='kernel_share', trace=os.path.basename(files[0]), kernel_time_ms=round(total / 1e6, 3),
                heads_share=round(heads / total, 4) if total else None, heads_ms={k: round(v / 1e6, 3) for k, v in rows.items()}, top=top,
                note='totals over the traced run: the frame is rendered once, then 3 warm-up steps and --reps timed ones')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'heads_train.jsonl'))
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true', help='time the kernel variant alone (for a kernel trace)')
    ap.add_argument('--share', help='directory of a rocprofv3 --kernel-trace --stats run of this script')
    ap.add_argument('--regularisers', action='store_true', help='time the regularised step (default --out profiles/relight_reg.jsonl)')
    ap.add_argument('--light-noise', action='store_true', help='time the regularised step under light-position noise (default --out profiles/light_noise.jsonl)')
    args = ap.parse_args()
    if args.light_noise and args.out == os.path.join('profiles', 'heads_train.jsonl'):
        args.out = os.path.join('profiles', 'light_noise.jsonl')
    if args.regularisers and args.out == os.path.join('profiles', 'heads_train.jsonl'):
        args.out = os.path.join('profiles', 'relight_reg.jsonl')
    if args.share:
        line = json.dumps(share(args.share))
    else:
        from relightableavatar_amd import fitting, synthetic
        from relightableavatar_amd.config import make_cfg
        from relightableavatar_amd.networks import make_network
        from relightableavatar_amd.renderer import make_renderer
        assert torch.cuda.is_available(), 'needs an MI355X'
        dev = torch.device('cuda:0')
        cfg = make_cfg('novel_light')
        net = make_network(cfg)
        net.load_state_dict(synthetic.make_state_dict(0, relight=True, cfg=cfg))
        net = net.to(dev).eval()
        batch = synthetic.to_device(synthetic.make_batch(args.size, args.size, seed=0, posed=True, n_novel_lights=1), dev)
        renderer = make_renderer(cfg, net)
        maps = renderer.render(batch)['probe00']
        eng = net.engine()
        probe = batch.novel_lights['probe00'].probe
        probe = (probe[0] if probe.ndim == 4 else probe).to(dev).float()
        with torch.no_grad():
            cache = [fitting._frame_cache(eng, cfg, batch, maps, maps.rgb_map.reshape(-1, 3) * 0.9, None, True)]
        theta = eng.heads_params().requires_grad_(True)
        if args.regularisers or args.light_noise:
            if args.light_noise:
                again = synthetic.to_device(synthetic.make_batch(args.size, args.size, seed=0, posed=True, n_novel_lights=1), dev)
                box = again.wbounds.clone()

                def fresh():
                    again.wbounds.copy_(box)          # the renderer grows the box in place
                    renderer.render(again)
                line = json.dumps(light_noise_leg(args, eng, cfg, net, batch, maps, theta, probe, fitting, fresh))
            else:
                line = json.dumps(regularised_leg(args, eng, cfg, cache, theta, probe, fitting))
            print(line, flush=True)
            if args.out and args.out != '/dev/null':
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, 'a') as f:
                    f.write(line + '\n')
            return

        def step(heads):
            theta.grad = None
            fitting.heads_loss(eng, cache, theta, probe, heads).backward()
        variants = [('kernels', fitting.material_heads)] + ([] if args.kernels_only else [('torch_fp32', torch_heads)])
        for _ in range(3):
            for _, h in variants:
                step(h)
        torch.cuda.synchronize()
        t = {k: [] for k, _ in variants}
        for _ in range(args.reps):
            for k, h in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(h)
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1))
        r = dict(tool='bench_heads', kind='step', size=args.size, hit_pixels=int(cache[0].w.shape[0]), samples=int(cache[0].feat.shape[0]),
                 reps=args.reps, device=torch.cuda.get_device_name(0))
        for k, v in t.items():
            r[k + '_step_ms'] = round(median(v), 4)
            r[k + '_step_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        if 'torch_fp32' in t:
            r['kernels_over_torch'] = round(r['kernels_step_ms'] / r['torch_fp32_step_ms'], 3)
        r['note'] = 'one loss + backward of fit_heads without the Adam update; composite, ra_reshade and ra_reshade_backward are common to both'
        line = json.dumps(r)
    print(line, flush=True)
    if args.out and args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""CPU-only tests: the C-ABI library loads and exports every declared symbol, host-side mirror classes
keep the reference's state_dict keys, chunking/sharding logic (incl. a world_size-2 gloo run)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from relightableavatar_amd import _lib, shard, synthetic
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.renderer.chunking import chunks

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(REPO, 'include', 'relightableavatar.h')).read()
    declared = set(re.findall(r'^(?:int|const char\*)\s+(ra_[a-z0-9_]+)\s*\(', hdr, flags=re.M))
    assert declared, 'no declarations found'
    for name in declared:
        assert hasattr(L, name), f'{name} declared in the header but not exported'
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert L.ra_abi_version() == _lib.ABI_VERSION == int(re.search(r'#define RA_ABI_VERSION (\d+)', hdr).group(1))


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from relightableavatar_amd.engine import Engine
    with pytest.raises(_lib.RaError, match='no CPU fallback'):
        Engine(make_cfg('relight'))
    from relightableavatar_amd.networks import make_network
    net = make_network(make_cfg('relight'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.inference_world_distance_field(torch.zeros(1, 4, 3), synthetic.make_body(0))


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, 'relightableavatar_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(root, f)).read()
                imports = [l for l in src.split('\n') if re.match(r'\s*(from|import)\s', l)]
                assert not any('oracle' in l for l in imports), f'{f} imports the oracle'
                # synthetic.py is the benchmark's / tests' input generator (weights, body, camera): the render path must not depend on it
                assert f == 'synthetic.py' or not any('synthetic' in l for l in imports), f'{f} imports the synthetic test-data module'


@pytest.mark.parametrize('mode,relight,n', [('anisdf', False, 64), ('relight', True, 82)])
def test_state_dict_keys_match_reference(mode, relight, n):
    from relightableavatar_amd.networks import make_network
    cfg = make_cfg(mode)
    net = make_network(cfg)
    sd = synthetic.make_state_dict(0, relight=relight, cfg=cfg)     # keys validated against the reference in make_golden.py
    assert len(net.state_dict()) == n
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert net.signed_distance_network.mlp.lin3.weight_v.shape == (205, 256)
    assert net.signed_distance_network.mlp.lin8.weight_v.shape == (257, 256)
    assert net.residual_deformation_network.mlp.linears[4].weight.shape == (256, 475)
    assert net.render_network.l3.weight_v.shape == (256, 412)
    if relight:
        assert net.global_env_map.shape == (32, 64, 3) and net.light_xyz.shape == (16, 32, 3)
        assert abs(float(net.light_area.sum()) - 4 * 3.14159265) < 1e-4


def test_chunk_rule():
    assert chunks(0, 8192) == []
    assert chunks(100, 8192) == [(0, 100)]
    assert chunks(262144, 65536) == [(0, 65536), (65536, 131072), (131072, 196608), (196608, 262144)]
    c = chunks(150000, 65536)          # ceil(150000 / 3) = 50000
    assert c == [(0, 50000), (50000, 100000), (100000, 150000)]


def test_make_cfg_modes():
    c = make_cfg('relight')
    assert c.dist_th == 0.125 and c.obj_lvis.dist_th == 0.125 and c.n_samples == 3 and c.render_chunk_size == 65536
    assert c.renderer_module.endswith('sphere_tracing_renderer') and c.network_module.endswith('relight_network')
    c = make_cfg('anisdf')
    assert c.n_samples == 128 and c.render_chunk_size == 8192 and c.dist_th == 0.1
    assert make_cfg('novel_light').renderer_module.endswith('novel_light_sphere_tracing')
    with pytest.raises(ValueError):
        make_cfg('nope')


def test_shard_roundtrip_single_process():
    P, world = 1003, 4
    x = torch.arange(P * 3, dtype=torch.float32).view(1, P, 3)
    idx = [shard.shard_indices(P, r, world) for r in range(world)]
    assert sorted(torch.cat(idx).tolist()) == list(range(P))
    b = synthetic.make_batch(32, 32, seed=0)
    s0 = shard.shard_batch(b, 0, 2)
    assert abs(s0.ray_o.shape[1] - b.ray_o.shape[1] / 2) <= 64 and s0.wbounds is not b.wbounds


def test_shard_tiles_partition_the_frame():
    """pixels are dealt to ranks in 8x8 tiles (waves of 64 neighbouring rays stay compact on every rank); the
    shards partition the in-box rays and are balanced"""
    b = synthetic.make_batch(128, 128, seed=0)
    P = b.ray_o.shape[1]
    H = W = 128
    for world in (2, 4, 8):
        owner = shard.ray_owner(P, world, b)
        pix = b.mask_at_box.reshape(-1).nonzero()[:, 0]
        tile = ((pix // W) // shard.TILE) * (W // shard.TILE) + (pix % W) // shard.TILE
        for t in tile.unique()[:50].tolist():
            assert owner[tile == t].unique().numel() == 1            # a tile never straddles ranks
        idx = [shard.shard_indices(P, r, world, b) for r in range(world)]
        assert sorted(torch.cat(idx).tolist()) == list(range(P))
        sizes = torch.tensor([i.numel() for i in idx], dtype=torch.float32)
        assert float(sizes.max() / sizes.mean()) < 1.25
        x = torch.rand(1, P, 3)
        parts = [x[:, i] for i in idx]                               # what each rank would hold
        pl = shard.plan(P, world, b)
        stacked = torch.zeros(world * pl.n_max, 3)
        for r in range(world):
            stacked[r * pl.n_max:r * pl.n_max + parts[r].shape[1]] = parts[r][0]
        full = torch.empty(P, 3)
        full[pl.order] = stacked[pl.src]
        assert torch.equal(full, x[0])                               # the exchange's index vectors invert the sharding


WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from relightableavatar_amd import shard
from relightableavatar_amd.base_utils import dotdict
dist.init_process_group('gloo')
rank, world = dist.get_rank(), dist.get_world_size()
P = 1001
g = torch.Generator().manual_seed(0)
ray = torch.rand(1, P, 3, generator=g)
batch = dotdict(ray_o=ray, ray_d=ray * 2, near=ray[..., 0], far=ray[..., 1], wbounds=torch.zeros(1, 2, 3))
class FakeRenderer:                       # per-ray function of the inputs: stands in for the GPU renderer
    def render(self, b):
        return dotdict(rgb_map=b.ray_o * 3 + b.ray_d, acc_map=b.near + b.far)
out = shard.render_sharded(FakeRenderer(), batch, ('rgb_map', 'acc_map'), rank, world)
ref = FakeRenderer().render(batch)
assert out.rgb_map.shape == (1, P, 3) and out.acc_map.shape == (1, P)
assert torch.equal(out.rgb_map, ref.rgb_map) and torch.equal(out.acc_map, ref.acc_map)
dist.destroy_process_group()
print('rank', rank, 'ok')
'''


WORKER_GROUND = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from relightableavatar_amd import shard, synthetic
from relightableavatar_amd.base_utils import dotdict
dist.init_process_group('gloo')
rank, world = dist.get_rank(), dist.get_world_size()
batch = synthetic.make_batch(96, 96, seed=0)
P, F = batch.ray_o.shape[1], 96 * 96
class FakeGroundRenderer:                 # stands in for the sphere-tracing renderer with cfg.vis_ground_shading: full-frame maps of the
    cfg = dotdict(vis_ground_shading=True, render_chunk_size=2000)          # rank's ground pixels, its human rays blended in at their pixels
    def render(self, b):
        pix = b.get('ground_pix', None)
        inds = b.ground_inds if pix is not None else b.mask_at_box.reshape(-1).nonzero()[:, 0]
        pix = torch.arange(F) if pix is None else pix
        g = pix.float()[:, None] * torch.tensor([1.0, 2.0, 3.0])
        g[inds] += b.ray_o[0] * 7 + b.far[0][:, None]
        b.mask_at_box[:] = True                                             # the real ground pass does (:1103)
        return dotdict(rgb_map=g[None], acc_map=(pix.float() * 0.5)[None])
ref = FakeGroundRenderer().render(dotdict(batch, mask_at_box=batch.mask_at_box.clone()))
out = shard.render_sharded(FakeGroundRenderer(), batch, ('rgb_map', 'acc_map'), rank, world)
assert out.rgb_map.shape == (1, F, 3) and out.acc_map.shape == (1, F)
assert torch.equal(out.rgb_map, ref.rgb_map) and torch.equal(out.acc_map, ref.acc_map)
assert not batch.mask_at_box.all()                                          # the caller's mask is untouched
dist.destroy_process_group()
print('rank', rank, 'ok')
'''


def test_sharded_ground_pass_gloo_world2(tmp_path):
    """the N > 1 path of the README command (ground-plane pass): every rank renders its full-frame tiles with its human rays
    blended in locally, ONE all_gather assembles the frame"""
    script = tmp_path / 'worker_ground.py'
    script.write_text(WORKER_GROUND)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', '29613', str(script), REPO], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('ok') == 2


def test_sharded_render_gloo_world2(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', '29611', str(script), REPO], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('ok') == 2


def test_bench_launcher_starts_n_ranks():
    """`python bench.py --gpus 2` outside torchrun is a launcher: it starts 2 ranks under torch.distributed.run, which shard the
    frame, gather it (gloo here, RCCL on the GPU box) and print ONE JSON line with n_gpus = 2 (--dry: no HIP engine)"""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--dry', '--size', '96', '--steps', '2',
                        '--warmup', '1'], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['steps'] == 2 and line['value'] > 0 and line['config']['gather_ok'] is True
    # and the rank program refuses a world size that contradicts --gpus
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '4', '--dry', '--backend', 'gloo'], capture_output=True, text=True,
                       env=dict(env, RANK='0', WORLD_SIZE='2', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29655'), timeout=300)
    assert r.returncode != 0 and 'WORLD_SIZE' in (r.stdout + r.stderr)


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every map of the last step as float32 <name>.npy; past the byte budget all maps keep the same seeded
    sample of rays (listed in sample_rays.npy), identical from run to run"""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    from relightableavatar_amd.base_utils import dotdict
    g = torch.Generator().manual_seed(1)
    maps = dotdict(rgb_map=torch.rand(1, 1000, 3, generator=g, dtype=torch.float16), acc_map=torch.rand(1, 1000, generator=g), note='not an array')
    bench.dump_outputs(str(tmp_path / 'a'), maps, 'out')
    assert sorted(os.listdir(tmp_path / 'a')) == ['acc_map.npy', 'rgb_map.npy']
    rgb = np.load(tmp_path / 'a' / 'rgb_map.npy')
    assert rgb.dtype == np.float32 and np.array_equal(rgb, maps.rgb_map.float().numpy())
    bench.dump_outputs(str(tmp_path / 't'), maps.acc_map, 'rgb_probes')
    assert np.array_equal(np.load(tmp_path / 't' / 'rgb_probes.npy'), maps.acc_map.numpy())
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4000)
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), maps, 'out')
    keep = np.load(tmp_path / 'b' / 'sample_rays.npy').astype(np.int64)
    assert 0 < len(keep) < 1000 and np.array_equal(keep, np.load(tmp_path / 'c' / 'sample_rays.npy'))
    got = {k: np.load(tmp_path / 'b' / f'{k}.npy') for k in ('rgb_map', 'acc_map')}
    assert sum(a.nbytes for a in got.values()) <= 4000
    assert np.array_equal(got['rgb_map'], rgb[:, keep]) and np.array_equal(got['acc_map'], maps.acc_map.numpy()[:, keep])


@pytest.mark.parametrize('extra', [[], ['--ground', '--mode', 'novel_light', '--probes', '2']])
def test_frames_in_flight_keep_their_collectives_apart_gloo_world4(extra):
    """Four ranks, THREE frames in flight in one process group (bench.py --dry --frames-in-flight 3: the gathers of frames f, f + 1, f + 2
    are outstanding when frame f is collected, as the replica streams of pipeline.py leave them on the GPU).  Every frame carries its own
    payload factor, every rank checks every gathered frame against ITS frame: the collectives run in submission order on all ranks and
    no frame picks up a neighbour's shards (gloo here; what RCCL's internal stream does with them is the hardware run's to show)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '4', '--backend', 'gloo', '--dry', '--size', '96', '--steps', '7',
                        '--warmup', '2', '--frames-in-flight', '3'] + extra, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert line['n_gpus'] == 4 and line['ranks_seen'] == 4 and line['config']['gather_ok'] is True and line['config']['frames_in_flight'] == 3
    assert len(line['per_rank']['rays_per_frame']) == 4 and sum(line['per_rank']['rays_per_frame']) > 0


def test_shards_carry_the_frames_chunk_boundaries():
    """quirk 1 (per-chunk growth of batch.wbounds): a shard renders its rays chunk by chunk of the WHOLE frame"""
    b = synthetic.make_batch(96, 96, seed=0)
    P = b.ray_o.shape[1]
    chunk = 700
    full = chunks(P, chunk)
    for world in (2, 3):
        seen = torch.zeros(P, dtype=torch.long)
        for r in range(world):
            sb = shard.shard_batch(b, r, world, chunk)
            idx = shard.shard_indices(P, r, world, b)
            assert len(sb.render_chunks) == len(full)
            assert sb.render_chunks[0][0] == 0 and sb.render_chunks[-1][1] == idx.numel()
            for (a, e), (fa, fe) in zip(sb.render_chunks, full):
                assert bool(((idx[a:e] >= fa) & (idx[a:e] < fe)).all())               # those rays do belong to that frame chunk
                seen[idx[a:e]] += 1
        assert bool((seen == 1).all())
    assert 'render_chunks' not in shard.shard_batch(b, 0, 1, chunk)                  # world 1: the batch itself


def test_ground_pass_is_dealt_by_the_same_tiles():
    """the full-frame ground pass of a sharded frame: every rank's in-box (human) pixels are a subset of its ground pixels (so the
    alpha blend of the two layers is rank-local), the ground shards partition the frame, carry the frame's chunk boundaries, and
    the exchange's index vectors invert the deal"""
    b = synthetic.make_batch(96, 96, seed=0)
    P, F = b.ray_o.shape[1], 96 * 96
    pix = b.mask_at_box.reshape(-1).nonzero()[:, 0]
    for world in (2, 3, 8):
        pl = shard.make_plan(P, world, b, ground=True, render_chunk_size=2000)
        g = pl.ground
        assert sorted(torch.cat(g.idx).tolist()) == list(range(F))
        full_chunks = chunks(F, 2000)
        for r in range(world):
            sb = shard.shard_batch(b, r, world, 2000, pl, ground=True)
            assert torch.equal(sb.ground_pix[sb.ground_inds], pix[pl.idx[r]])        # its human rays, found among its ground pixels
            assert len(sb.ground_chunks) == len(full_chunks) and sb.ground_chunks[-1][1] == sb.ground_pix.numel()
            for (a, e), (fa, fe) in zip(sb.ground_chunks, full_chunks):
                assert bool(((sb.ground_pix[a:e] >= fa) & (sb.ground_pix[a:e] < fe)).all())
            assert sb.mask_at_box is not b.mask_at_box                                # the ground pass overwrites the shard's copy only
        x = torch.rand(F, 2)
        stacked = torch.zeros(world * g.n_max, 2)
        for r in range(world):
            stacked[r * g.n_max:r * g.n_max + g.idx[r].numel()] = x[g.idx[r]]
        full = torch.empty(F, 2)
        full[g.order] = stacked[g.src]
        assert torch.equal(full, x)


def test_plan_is_keyed_on_the_mask_content():
    """a new frame's mask at a recycled address, or an in-place edit of the live mask, must not hit another frame's
    plan — and the same content does, whatever tensor carries it.  use_cache=False always rebuilds (bench.py: a new frame per step)."""
    b1 = synthetic.make_batch(64, 64, seed=0)
    P = b1.ray_o.shape[1]
    p1 = shard.make_plan(P, 2, b1)
    assert shard.make_plan(P, 2, b1) is p1
    b2 = synthetic.make_batch(64, 64, seed=0)
    b2.mask_at_box = b1.mask_at_box.clone()
    assert shard.make_plan(P, 2, b2) is p1                                           # same content: same plan
    assert shard.make_plan(P, 2, b1, use_cache=False) is not p1
    m = b1.mask_at_box.reshape(-1)
    on = m.nonzero()[:, 0]
    m[on[0]] = False                                                                 # in-place edit: one in-box pixel less
    p3 = shard.make_plan(P - 1, 2, b1)
    assert p3 is not p1 and sum(p3.counts) == P - 1
    # a renderer that overwrites the mask between shard and gather (the ground pass does) cannot change the ownership: the plan is explicit
    pl = shard.make_plan(P, 2, b2)
    own = pl.idx[0].clone()
    sb = shard.shard_batch(b2, 0, 2, None, pl)
    b2.mask_at_box[:] = True
    assert sb.ray_o.shape[1] == pl.counts[0] and torch.equal(pl.idx[0], own)         # the plan in hand still describes the shard
    assert not sb.mask_at_box.all()                                                  # and the shard carries its own copy of the mask


def test_fixed_material_source_rule():
    """base_network.py:501-503 without a GPU: which pose conditions the colour net"""
    import types
    from relightableavatar_amd.engine import Engine
    body = synthetic.make_body(0)
    pick = lambda **kw: Engine._cond_fix_source(types.SimpleNamespace(relight=False, cfg=make_cfg('anisdf', **kw)), body)
    assert pick(fix_material=0) is body.train_motion.poses
    assert pick(fix_material=-1, always_fix_material=True) is body.train_motion.poses
    assert pick(fix_material=-1, always_fix_material=False) is body.poses
    nb = synthetic.make_body(0)
    del nb['train_motion']
    with pytest.raises(ValueError, match='train_motion'):
        Engine._cond_fix_source(types.SimpleNamespace(relight=False, cfg=make_cfg('anisdf')), nb)
    assert Engine._cond_fix_source(types.SimpleNamespace(relight=True, cfg=make_cfg('relight')), nb) is None


def test_lazydict_never_leaks_a_thunk():
    """advisor (round 3): dict(lazydict) / dotdict(lazydict) took CPython's fast path and copied raw thunks; the thunks of the renderers'
    per-hit outputs name the tensors they close over, so that pipeline.Pending.result can record them on the consumer's stream"""
    import copy
    import pickle
    from relightableavatar_amd.base_utils import dotdict, lazydict
    t = torch.arange(6.0)
    calls = []
    d = lazydict(a=1)
    d.lazy('b', lambda: (calls.append(1), t * 2)[1], deps=(t,))
    assert d.pending_tensors() == [t] and not calls
    for c in (dict(d), dotdict(d), copy.copy(d), pickle.loads(pickle.dumps(d))):
        assert torch.equal(c['b'], t * 2) and not isinstance(c['b'], lazydict._Thunk)
    assert len(calls) == 1 and d.pending_tensors() == []          # evaluated once, then a plain entry
    k = d.copy()
    assert isinstance(k, lazydict) and torch.equal(k.b, t * 2)


def test_to_device_keeps_the_bounds_mirror_valid():
    """advisor (round 3): to_device stored wbounds_host without its version, so the renderer discarded the mirror and read the box back
    (one stream sync per frame)"""
    from relightableavatar_amd import synthetic
    b = synthetic.to_device(synthetic.make_batch(32, 32, seed=0), torch.device('cpu'))
    assert 'wbounds_host' not in b or b.wbounds_host_version == b.wbounds._version
    b2 = synthetic.make_batch(32, 32, seed=0)
    b2.wbounds_host = b2.wbounds.clone()
    out = synthetic.to_device(b2, torch.device('cpu'))
    assert out.wbounds_host_version == out.wbounds._version


@pytest.mark.parametrize('extra', [['--mode', 'novel_light', '--probes', '8'], ['--mode', 'novel_light', '--probes', '8', '--ground'], ['--ground']])
def test_gather_of_the_novel_light_and_ground_payloads_gloo_world2(extra):
    """round-3 verdict, item 6c: the N > 1 exchange of config 5's payload (8 probes x rgb = 24 channels) and of the README command's
    full-frame ground maps, world size 2 over gloo: the gathered frame must equal the whole frame; the line must say how many ranks took
    part, what each did and how many bytes the gather moved"""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--dry', '--size', '96', '--steps', '2',
                        '--warmup', '1'] + extra, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert line['config']['gather_ok'] is True and line['ranks_seen'] == 2 and len(line['per_rank']['ms_per_step']) == 2
    C = 24 if 'novel_light' in extra else 4
    assert line['gather']['channels'] == C and line['gather']['bytes_received_per_rank'] >= (96 * 96 if '--ground' in extra else sum(line['per_rank']['rays_per_frame'])) * C * 4
    assert 0 <= line['gather']['pad_fraction'] < 0.1
    assert 'ms_per_step_sequential' in line


def test_ctypes_structs_match_the_header():
    """the ctypes mirrors of the C ABI's structs must have the header's layout: a field missing on the Python side makes the library read
    past the struct (found the hard way: ra_sphere_params.n_boxes).  Sizes and last-field offsets are compared with a C compiler's."""
    import ctypes as C
    import shutil
    import tempfile
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    structs = {'ra_config': 'clip_far', 'ra_frame': 'n_verts', 'ra_trace_params': 'dist_th', 'ra_render_out': 'volume_roughness',
               'ra_sphere_params': 'box_start', 'ra_ground_params': 'box_start', 'ra_ground_out': 'ldot', 'ra_pose_in': 'bounds_padding',
               'ra_pose_out': 'Th', 'ra_image_params': 'tbounds', 'ra_counters': 'n_fine_sdf_comp'}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "relightableavatar.h"\nint main(){\n' + \
          ''.join(f'printf("{n} %zu %zu\\n", sizeof({n}), offsetof({n}, {f}));\n' for n, f in structs.items()) + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.run(['gcc', '-I', os.path.join(REPO, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')], check=True)
        out = subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout
    for line in out.strip().splitlines():
        name, size, off = line.split()
        cls = getattr(_lib, name)
        assert C.sizeof(cls) == int(size), (name, C.sizeof(cls), size)
        assert getattr(cls, structs[name]).offset == int(off), (name, structs[name])


def test_native_plan_equals_the_numpy_plan():
    """shard.make_plan's per-frame part runs in ONE C call (ra_shard_plan, csrc/ra_shard.cpp: host code, no GPU); the numpy restatement
    it replaced stays as its checker: ownership, exchange index vectors, per-rank chunk ranges and ground-pass positions must agree
    element for element — odd frame sizes, masks with holes, 1 .. 8 ranks, with and without the ground pass and render chunks."""
    import numpy as np
    from relightableavatar_amd.base_utils import dotdict
    rng = np.random.default_rng(0)

    def same(a, b, path=''):
        if isinstance(a, dict):
            for k in a:
                if k.startswith('_') or k in ('ready', 'owner_host'):
                    continue
                assert k in b, (path, k)
                same(a[k], b[k], path + '/' + k)
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), (path, len(a), len(b))
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f'{path}[{i}]')
        elif torch.is_tensor(a):
            assert torch.equal(a.cpu(), torch.as_tensor(b).cpu()), path
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b)), path
        else:
            assert a == b, (path, a, b)

    try:
        for H, W in ((64, 64), (60, 52), (130, 67), (256, 256)):
            yy, xx = np.mgrid[0:H, 0:W]
            for world in (1, 2, 3, 8):
                for ground in (False, True):
                    for chunk in (None, 700, 65536):
                        m = ((yy - H / 2) ** 2 + (xx - W / 2.3) ** 2 < (0.3 * H) ** 2) & (rng.random((H, W)) > 0.1)
                        P = int(m.sum())
                        batch = dotdict(mask_at_box=torch.from_numpy(m.reshape(1, -1)), meta=dotdict(H=torch.tensor([H]), W=torch.tensor([W])))
                        shard._NUMPY_PLAN = False
                        a = shard.make_plan(P, world, batch, ground=ground, render_chunk_size=chunk, use_cache=False)
                        assert '_stage' in a                      # the native path ran
                        shard._NUMPY_PLAN = True
                        b = shard.make_plan(P, world, batch, ground=ground, render_chunk_size=chunk, use_cache=False)
                        same(dict(b), dict(a))
        # a mask that does not hold P pixels: no tile deal, runs of rays (both paths)
        shard._NUMPY_PLAN = False
        c = shard.make_plan(P - 1, 2, batch, use_cache=False)
        assert '_stage' not in c and sum(c.counts) == P - 1
    finally:
        shard._NUMPY_PLAN = False


def test_no_unsafe_packed_fp32_in_the_shipped_objects():
    """Round 5: on MI355X a packed fp32 instruction whose `op_sel` routes a HIGH source half into its LOW lane returns
    wrong low halves when its wave shares a SIMD with another wave's MFMAs (tools/pk_f32_hazard.hip) — what corrupted the skinning kernel of
    animated sequences with frames in flight.  The compiler's SLP vectoriser formed them; the library is built with -fno-slp-vectorize, and
    no object may contain the form (plain packed ops and op_sel_hi-only selects, the coarse level's hand-written scan, are clean)."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import check_packed_fp32
    objs = sorted(__import__('glob').glob(os.path.join(REPO, 'relightableavatar_amd', 'csrc', '*.o')))
    if not objs:
        pytest.skip('library objects not built in-tree')
    unsafe, report = check_packed_fp32.check(objs)
    assert unsafe == 0, report
    assert 'ra_hdq.o' in report           # the scan sees device code at all (the coarse level's hand-written packed fp32)


def test_packed_fp32_gate_fails_closed(tmp_path):
    """the link-time gate must not pass when it could not look (advisor, round 5): something that is no object file, a host-only object that
    claims a .hip source, an architecture the objects hold no code for — each is an error, not 'no unsafe instruction found'"""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import check_packed_fp32 as C
    junk = tmp_path / 'junk.o'
    junk.write_bytes(b'not an object file')
    with pytest.raises(C.CheckError):
        C.check([str(junk)])
    objs = sorted(__import__('glob').glob(os.path.join(REPO, 'relightableavatar_amd', 'csrc', 'ra_image.o')))
    if not objs:
        pytest.skip('library objects not built in-tree')
    with pytest.raises(C.CheckError, match='no device code object for gfx90a'):
        C.check(objs, arch='gfx90a')
    # a host-only object next to a .hip source of the same name: device code is missing, not absent by design
    import subprocess
    src = tmp_path / 'k.hip'
    src.write_text('int f() { return 1; }\n')
    obj = tmp_path / 'k.o'
    subprocess.run(['g++', '-x', 'c++', '-c', str(src), '-o', str(obj)], check=True)
    with pytest.raises(C.CheckError, match='holds no device code'):
        C.check([str(obj)])


def test_default_config_matches_the_python_defaults():
    """ra_default_config() (no ctx, no GPU) hands a C caller the documented defaults — a zero-initialised ra_config is NOT the default
    (trace_precision 0, clip_far 0: rejected by ra_set_config) — and they are the values make_cfg('relight') sends through the binding."""
    import ctypes as C
    from relightableavatar_amd.config import make_cfg
    c = _lib.ra_config()
    assert _lib.lib().ra_default_config(C.byref(c)) == 0
    cfg = make_cfg('relight')
    for k in ('xyz_res', 'sdf_res', 'view_res', 'n_bones', 'resd_limit', 'blend_radius', 'albedo_slope', 'albedo_bias', 'roughness_slope',
              'roughness_bias', 'fresnel_f0', 'shading_albedo', 'albedo_multiplier', 'bg_brightness', 'trace_precision',
              'k4_batch_slots', 'key_light_share'):
        assert abs(float(getattr(c, k)) - float(cfg[k])) < 1e-6, k
    assert c.relight == 1 and c.mlp_f16 == 1 and c.query_skip == 1 and c.tonemapping == 1 and c.lambert_only == 0 and c.glossy_only == 0
    assert abs(c.clip_near - 0.02) < 1e-7 and c.clip_far == 10.0
    assert c.only_visibility == 0 and c.vis_shade_map == 0 and c.use_geodesic_filter == 1
    assert not cfg.only_visibility and not cfg.vis_lvis_map and not cfg.vis_ldot_map and cfg.use_geodesic_filter


def test_k3cc_fragment_registers_are_only_touched_by_name():
    """K3CC (csrc/ra_k3cc.hpp) keeps 62 weight fragments in flight in AGPRs it addresses by name from inline assembly: the compiler must not
    write an AGPR anywhere else in that kernel, and may read one only after the counted wait that makes its load a value
    (tools/check_k3cc_isa.py compiles the kernel to gfx950 assembly with the product flags and checks exactly that)."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import check_k3cc_isa
    problems, stats = check_k3cc_isa.check()
    assert not problems, problems[:5]
    assert stats['agpr_reads'] == 8 * stats['waits']


def test_unsupported_reference_switches_are_refused_not_ignored():
    """switches of the reference's hot path this build does not reproduce (each cannot run in the reference release either, or needs a
    third-party CUDA extension) raise at make_network / make_renderer; at their defaults they pass"""
    from relightableavatar_amd import config
    from relightableavatar_amd.config import make_cfg
    config.check_supported(make_cfg('relight'))
    config.check_supported(make_cfg('relight', ablate_hdq_mode='hdq', bruteforce_st=False))
    for k, v in (('bruteforce_st', True), ('smpl_distance', True), ('ablate_hdq_mode', 'world'), ('check_bound_sdf', True), ('zero_roughness', True)):
        with pytest.raises(NotImplementedError, match=k):
            config.check_supported(make_cfg('relight', **{k: v}))
    from relightableavatar_amd.networks import make_network
    with pytest.raises(NotImplementedError):
        make_network(make_cfg('relight', smpl_distance=True))


def test_shard_plan_under_sanitizers(tmp_path):
    """the library's host-side C++ that runs every frame of a sharded job (csrc/ra_shard.cpp: plain C++, no HIP) built with
    -fsanitize=address,undefined and fuzzed against its contract: 3 000 random frames (empty / full / ragged masks, 1-9 ranks, with and
    without the ground pass's fixed stripes, random chunk edges, exact-size output blocks, wrong-P and null-argument error paths)"""
    import shutil
    import subprocess
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'shard_fuzz')
    src = os.path.join(REPO, 'tests', 'native', 'shard_fuzz.cpp')
    subprocess.run(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', exe], check=True)
    r = subprocess.run([exe, '3000'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'cases ok' in r.stdout, (r.stdout[-500:], r.stderr[-2000:])

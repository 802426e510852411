"""The mesh connectivity stages at the size of an extracted avatar: time per call (host clock around a device synchronise for the
build, which ends in its read-back; HIP events for the rest; warm clocks, one process).  The mesh is the synthetic template at 2 502
vertices subdivided three times onto its ellipsoid: 160 002 vertices, 320 000 faces, closed.  One JSON line per stage:

    build      Engine.topology: keys, radix sort, edge ids, twins, the two vertex lists, ONE read-back (counted and reported)
    smooth     Topology.smooth, 90 Taubin iterations of the positions (180 launches)
    subdivide  two chained Topology.subdivide steps of the positions (5.12 M faces at the end); the children come from index arithmetic

Beside each stage goes the same stage in plain torch ops on the device (this tool's own restatement: unique / argsort, an
index_add_ over the directed edges per pass), for scale only; its results are compared with the library's (integers exactly; positions by
their largest difference) and the line says so.

    python tools/bench_mesh_topology.py [--out profiles/mesh_topology.jsonl] [--reps 10]

Every leg is warmed up (code objects, ctx scratch, the caching allocator, clocks), then timed `reps` times, the legs interleaved;
the median and the spread are reported.  No target is fixed: the numbers are written down.  A run without a HIP device fails: there
is no CPU fallback.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_mesh_distance import SCALE, stats, subdivide, template, timed
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ---------------------------------------------------------------------------------------------- the torch legs
def torch_build(faces, V):
    """unique edges, every half-edge's edge, twins of the manifold edges"""
    vert = faces.reshape(-1).long()
    nxt = faces.roll(-1, dims=1).reshape(-1).long()
    key = torch.minimum(vert, nxt) * V + torch.maximum(vert, nxt)
    u, edge, counts = key.unique(return_inverse=True, return_counts=True)
    order = edge.argsort(stable=True)
    twin = torch.full_like(edge, -1)
    pair = counts[edge[order]] == 2
    o = order[pair]
    twin[o[0::2]], twin[o[1::2]] = o[1::2], o[0::2]
    return torch.stack([u // V, u % V], 1), edge, twin


def torch_smooth(v, edges, alpha, iters):
    V = v.shape[0]
    idx = torch.cat([edges, edges.flip(1)]).t()
    deg = torch.zeros(V, device=v.device).index_add_(0, idx[0], torch.ones(idx.shape[1], device=v.device))
    w = (1.0 / deg[idx[0]])[:, None]
    mean = lambda x: torch.zeros_like(x).index_add_(0, idx[0], x[idx[1]] * w)
    for _ in range(iters):
        v = v + alpha * (mean(v) - v)
        v = v - (alpha + 0.01) * (mean(v) - v)
    return v


def torch_loop_step(v, faces, edge, E):
    """one Loop step of a CLOSED manifold mesh: vertices, faces"""
    V = v.shape[0]
    vert = faces.reshape(-1).long()
    nxt, prv = faces.roll(-1, dims=1).reshape(-1).long(), faces.roll(1, dims=1).reshape(-1).long()
    n = torch.zeros(V, device=v.device).index_add_(0, vert, torch.ones(vert.shape[0], device=v.device))
    beta = (1 / n) * (0.625 - (0.375 + 0.25 * torch.cos(2 * math.pi / n)) ** 2)
    out = torch.zeros(V + E, v.shape[1], device=v.device)
    out.index_add_(0, V + edge, (3 * v[vert] + v[prv]) / 8)
    out.index_add_(0, vert, (1 / n - beta)[vert, None] * v[vert] + beta[vert, None] * v[nxt])
    m = (V + edge).reshape(-1, 3)
    a, b, c = faces.long().t()
    corner = torch.stack([torch.stack(t, 1) for t in ((a, m[:, 0], m[:, 2]), (b, m[:, 1], m[:, 0]), (c, m[:, 2], m[:, 1]))], 1).reshape(-1, 3)
    return out, torch.cat([corner, torch.stack((m[:, 2], m[:, 0], m[:, 1]), 1)])       # the library's face order: 3 f + k, then the middle faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'mesh_topology.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--iters', type=int, default=90)
    ap.add_argument('--steps', type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    dev = eng.device
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    tv, tf = torch.from_numpy((v * SCALE).astype(np.float32)).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    V, F = tv.shape[0], tf.shape[0]
    base = dict(tool='bench_mesh_topology', verts=V, faces=F, reps=args.reps, device=torch.cuda.get_device_name(0))

    def lib_build():
        eng.topology(tf, V).close()

    def lib_loop(topo0):
        x, t, made = tv, topo0, []
        for _ in range(args.steps):
            x, fc, t = t.subdivide(x)
            made.append(t)
        return x, fc, made

    print(f'mesh: {V} vertices, {F} faces; warming up', file=sys.stderr, flush=True)
    # warm-up of every leg, and the answers to compare
    lib_build()
    topo = eng.topology(tf, V)
    edges_t, edge_t, twin_t = torch_build(tf, V)
    same_build = bool(torch.equal(edges_t, topo.edges) and torch.equal(edge_t, topo.array('edge')) and torch.equal(twin_t, topo.array('twin')))
    sm, sm_t = topo.smooth(tv, None, 0.33, args.iters), torch_smooth(tv, edges_t, 0.33, args.iters)
    sub, sub_f, made = lib_loop(topo)
    x, fc, ed, E = tv, tf, edge_t, topo.E
    for _ in range(args.steps):
        x, fc = torch_loop_step(x, fc, ed, E)
        _, ed, _ = torch_build(fc, x.shape[0])
        E = int(ed.max()) + 1
    torch.cuda.synchronize()
    loop_diff = float((sub[sub_f.long()] - x[fc]).abs().max())
    for t in made:
        t.close()
    legs = {k: [] for k in ('build', 'build_torch', 'smooth', 'smooth_torch', 'subdivide', 'subdivide_torch')}

    def torch_loop():
        x, fc, ed, E = tv, tf, edge_t, topo.E
        for k in range(args.steps):
            x, fc = torch_loop_step(x, fc, ed, E)
            if k + 1 < args.steps:      # the next level's edges: what a step without the half-edge arithmetic has to rebuild
                _, ed, _ = torch_build(fc, x.shape[0])
                E = int(ed.max()) + 1

    def lib_loop_timed():
        for t in lib_loop(topo)[2]:
            t.close()
    print('timing', file=sys.stderr, flush=True)
    for _ in range(args.reps):
        legs['build'].append(host_timed(lib_build))
        legs['build_torch'].append(host_timed(lambda: torch_build(tf, V)))
        legs['smooth'].append(timed(lambda: topo.smooth(tv, None, 0.33, args.iters)))
        legs['smooth_torch'].append(timed(lambda: torch_smooth(tv, edges_t, 0.33, args.iters)))
        legs['subdivide'].append(host_timed(lib_loop_timed))
        legs['subdivide_torch'].append(host_timed(torch_loop))
    lines = []
    for stage, extra in (('build', dict(edges=topo.E, max_valence=topo.max_valence, readbacks=topo.readbacks, equals_torch=same_build, clock='host, synchronised')),
                         ('smooth', dict(iters=args.iters, launches=2 * args.iters, readbacks=0, max_diff_torch=float((sm - sm_t).abs().max()), clock='device events')),
                         ('subdivide', dict(steps=args.steps, out_verts=int(sub.shape[0]), out_faces=int(sub_f.shape[0]), readbacks=0, max_corner_diff_torch=loop_diff,
                                            clock='host, synchronised; includes destroying the children'))):
        line = dict(base, stage=stage, **extra)
        stats(line, stage, legs[stage])
        stats(line, stage + '_torch', legs[stage + '_torch'])
        line['torch_over_lib'] = round(line[stage + '_torch_ms'] / line[stage + '_ms'], 2)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

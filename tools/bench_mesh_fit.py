"""The mesh-fitting stages at the size of an extracted avatar (the mesh of tools/bench_mesh_topology.py: 160 002 vertices, 320 000
faces, closed), HIP events around warm calls, one process.  One JSON line per stage:

    solve        Topology.diffuse_solve of M v (3 channels) at lambda = 9 and 29, tol 1e-9: the iterations it used, the time with exactly
                 that many iterations queued, the time per iteration, and the time with the default 256 queued — the difference is the
                 idle tail, launches that find their channel stopped and return
    adam         one AdamUniform step of the 3 V parameters
    fit          one iteration of bidirectional_icp_fitting (two meshes 0.005 apart, boundary_focus off): the difference between runs of
                 1 and of 1 + n iterations, host clock around a device synchronise, and its parts timed one by one

Beside the solve and the optimiser step goes the same algorithm in plain torch device ops (this tool's own restatement: a float64 CSR
sparse-mm Jacobi-preconditioned CG of the same number of iterations without read-back; an elementwise Adam with one amax), for scale;
the results are compared and the line says by how much they differ.  The fitting iteration has no torch leg: its closest-point query
has no torch form at this size.

    python tools/bench_mesh_fit.py [--out profiles/mesh_fit.jsonl] [--reps 10]

No target is fixed: the numbers are written down.  A run without a HIP device fails: there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_mesh_distance import SCALE, stats, subdivide, template, timed
from relightableavatar_amd import largesteps, mesh_utils
from relightableavatar_amd.config import make_cfg
from relightableavatar_amd.engine import Engine


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_matrix(edges, V, lam):
    """M = I + lam (D - A) as a float64 CSR tensor, and its diagonal"""
    i = torch.cat([edges[:, 0], edges[:, 1]])
    j = torch.cat([edges[:, 1], edges[:, 0]])
    deg = torch.zeros(V, dtype=torch.float64, device=edges.device).index_add_(0, i, torch.ones(i.shape[0], dtype=torch.float64, device=edges.device))
    diag = 1.0 + lam * deg
    ar = torch.arange(V, device=edges.device)
    M = torch.sparse_coo_tensor(torch.stack([torch.cat([i, ar]), torch.cat([j, ar])]), torch.cat([torch.full_like(i, -lam, dtype=torch.float64), diag]), (V, V))
    return M.coalesce().to_sparse_csr(), diag


def torch_cg(M, diag, b, iters):
    """`iters` iterations of Jacobi-preconditioned CG on float64 columns, every scalar kept on the device"""
    x = torch.zeros_like(b)
    r = b.clone()
    z = r / diag[:, None]
    p = z.clone()
    rz = (r * z).sum(0)
    for _ in range(iters):
        q = M @ p
        alpha = rz / (p * q).sum(0)
        x = x + alpha * p
        r = r - alpha * q
        z = r / diag[:, None]
        rz_new = (r * z).sum(0)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


def torch_adam(p, g, g1, g2, t, lr=0.1, b1=0.9, b2=0.999):
    g1.mul_(b1).add_(g, alpha=1 - b1)
    g2.mul_(b2).add_((1 - b2) * (g * g).amax())
    p.sub_(lr * (g1 / (1 - b1 ** t)) / (1e-8 + (g2 / (1 - b2 ** t)).sqrt()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'mesh_fit.jsonl'))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--subdivisions', type=int, default=3)
    ap.add_argument('--fit-iters', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    eng = Engine(make_cfg('relight'), device='cuda:0')
    dev = eng.device
    v, f = template(2502)
    for _ in range(args.subdivisions):
        v, f = subdivide(v, f)
    tv, tf = torch.from_numpy((v * SCALE).astype(np.float32)).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
    V, F = tv.shape[0], tf.shape[0]
    base = dict(tool='bench_mesh_fit', verts=V, faces=F, reps=args.reps, device=torch.cuda.get_device_name(0))
    topo = eng.topology(tf, V)
    lines = []
    print(f'mesh: {V} vertices, {F} faces', file=sys.stderr, flush=True)

    for lam in (9.0, 29.0):
        b = topo.diffuse_apply(tv, lam)
        x, info = topo.diffuse_solve(b, lam, info=True)
        iters = int(info.iters.max())
        M, diag = torch_matrix(topo.edges, V, lam)
        xt = torch_cg(M, diag, b.double(), iters)
        legs = {k: [] for k in ('solve', 'solve_default', 'solve_torch', 'apply')}
        for _ in range(args.reps):
            legs['solve'].append(timed(lambda: topo.diffuse_solve(b, lam, max_iter=iters)))
            legs['solve_default'].append(timed(lambda: topo.diffuse_solve(b, lam)))
            legs['solve_torch'].append(timed(lambda: torch_cg(M, diag, b.double(), iters)))
            legs['apply'].append(timed(lambda: topo.diffuse_apply(tv, lam)))
        line = dict(base, stage='solve', lam=lam, channels=3, tol=1e-9, iters=info.iters.tolist(), residual=float(info.residual.max()), launches_per_iter=4,
                    readbacks=0, max_diff_torch=float((x.double() - xt).abs().max()), round_trip_error=float((x - tv).abs().max()), clock='device events')
        for k in legs:
            stats(line, k, legs[k])
        line['ms_per_iter'] = round(line['solve_ms'] / iters, 5)
        line['idle_tail_ms'] = round(line['solve_default_ms'] - line['solve_ms'], 4)
        line['idle_us_per_queued_iter'] = round(1e3 * line['idle_tail_ms'] / max(256 - iters, 1), 3)
        line['torch_over_lib'] = round(line['solve_torch_ms'] / line['solve_ms'], 2)
        lines.append(line)

    # the optimiser step
    n = 3 * V
    g = torch.randn(V, 3, device=dev) * 1e-3
    pa, ga1, ga2 = tv.clone(), torch.zeros_like(tv), torch.zeros(1, device=dev)
    pb, gb1, gb2 = tv.clone(), torch.zeros_like(tv), torch.zeros(1, device=dev)
    eng.adam_uniform_step(pa, g, ga1, ga2, 1, 3e-2)
    torch_adam(pb, g, gb1, gb2, 1, 3e-2)
    diff = float((pa - pb).abs().max())
    legs = {'adam': [], 'adam_torch': []}
    for k in range(args.reps):
        legs['adam'].append(timed(lambda: eng.adam_uniform_step(pa, g, ga1, ga2, k + 2, 3e-2)))
        legs['adam_torch'].append(timed(lambda: torch_adam(pb, g, gb1, gb2, k + 2, 3e-2)))
    line = dict(base, stage='adam', params=n, launches=2, max_diff_torch_after_one_step=diff, clock='device events')
    stats(line, 'adam', legs['adam'])
    stats(line, 'adam_torch', legs['adam_torch'])
    line['torch_over_lib'] = round(line['adam_torch_ms'] / line['adam_ms'], 2)
    lines.append(line)

    # one fitting iteration, and its parts
    nrm = topo.normals(tv, want=('vert_normal',)).vert_normal
    tv1 = (tv + 0.005 * nrm).contiguous()
    tf_host = tf.cpu()
    fit = lambda k: mesh_utils.bidirectional_icp_fitting(tv, tf_host, tv1, tf_host, 29, k, 1 << 30, 2e-4, boundary_focus=False, engine=eng, verbose=False)
    fit(1)
    one, many = [], []
    for _ in range(max(args.reps // 3, 2)):
        one.append(host_timed(lambda: fit(1)))
        many.append(host_timed(lambda: fit(1 + args.fit_iters)))
    per_iter = [(m - o) / args.fit_iters for o, m in zip(one, many)]
    Mx = largesteps.compute_matrix(tv, tf, 29, engine=eng)
    p = Mx.apply(tv)
    mesh = eng.mesh(tv1, tf_host)
    fn1 = topo.normals(tv1, want=('face_normal',)).face_normal
    parts = {k: [] for k in ('warm_solve', 'normals', 'mesh_build', 'icp_residual', 'cold_solve_of_gradient')}
    res = mesh.icp_residual(tv, nrm, fn1)
    for _ in range(args.reps):
        parts['warm_solve'].append(timed(lambda: Mx.solve(p, x0=tv)))
        parts['normals'].append(timed(lambda: topo.normals(tv, want=('face_normal', 'vert_normal'))))
        parts['mesh_build'].append(host_timed(lambda: eng.mesh(tv1, tf_host).close()))
        parts['icp_residual'].append(timed(lambda: mesh.icp_residual(tv, nrm, fn1)))
        parts['cold_solve_of_gradient'].append(timed(lambda: Mx.solve(res.grad)))
    line = dict(base, stage='fit', lam=29, kept=int(res.sums[1]), loss=float(res.loss), fit_iters=args.fit_iters,
                clock='host, synchronised, difference of two runs; parts: device events (mesh_build: host, with its destroy)')
    stats(line, 'fit_iteration', per_iter)
    for k in parts:
        stats(line, k, parts[k])
    lines.append(line)
    mesh.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for line in lines:
            s = json.dumps(line)
            print(s)
            fh.write(s + '\n')


if __name__ == '__main__':
    main()

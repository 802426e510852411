"""Device-side mirror of the reference's mesh evaluator: Chamfer and point-to-surface (P2S) distance between a predicted mesh and a scan.

    Evaluator.evaluate(output, batch), Evaluator.summarize()      lib/evaluators/mesh_evaluator.py:12-33
    MeshEvaluator.get_chamfer_dist, get_surface_dist              lib/evaluators/mesh_evaluator.py:62-98
    cfg.evaluator_module (mesh_cfg)                               configs/base.yaml:119-123

Per frame, in the reference's order: 1000 samples of the source surface, 1000 of the target's, the two closest-point queries
(Engine.mesh: ra_mesh_closest), chamfer = the mean of the two mean distances; then 10 000 fresh source samples and p2s = their mean
distance to the target.  Distances are sqrt(d2) taken to double before the mean.  evaluate() queues everything on the device into one
growing (N, 2) float64 table and reads no result back; summarize() does the only copy of results to the host, returns the two means,
keeps the per-frame lists in self.metrics (what the reference saves as chamfer.npy / p2s.npy) and resets.  There is no CPU fallback.
Two things in evaluate() do wait, and are not results: ra_mesh_create checks the faces on the HOST, so faces that arrive on the device
(the mesh renderer's keys) are copied back once per mesh — faces that arrive on the host (a path, numpy arrays, a trimesh object) are
used where they are and only a copy of them goes to the device for the sampling; and the frame's two meshes are released when it
is done, which waits for the device (ra_mesh_destroy).

Scope, stated rather than implied:
  - Sampling is trimesh.sample.sample_surface's method (mesh_utils.sample_surface) on torch's generator: the same distribution, not
    numpy's global random stream.  generator= makes a run reproducible.
  - The reference zeroes NaN distances (:76-77, 94).  trimesh produces them for degenerate faces; here every division is guarded and
    finite inputs give finite distances, so there is nothing to zero and nothing is.
  - output['mesh'] is anything with .vertices / .faces (a trimesh.Trimesh), or a mapping with the verts / faces keys that the mesh
    renderer returns (mesh_renderer.py:148-154), a leading batch dimension of 1 allowed.  batch['obj'][0] is a path (mesh_utils.load_obj:
    triangles only) or a (verts, faces) pair.
  - Writing p2s.npy / chamfer.npy stays out, as the metrics.npy of the image evaluator does.
  - MeshEvaluator's set_mesh (two paths), apply_registration (trimesh.registration) and scale_factor / offset, which the reference's
    Evaluator never uses, are not mirrored.
"""
import numpy as np
import torch

from .. import mesh_utils


def _as_mesh(mesh, who):
    """(verts (V,3), faces (F,3)) tensors of a mesh-like object, a mapping with verts / faces, a pair or a path"""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, '__fspath__'):
        return mesh_utils.load_obj(mesh)
    if hasattr(mesh, 'vertices') and hasattr(mesh, 'faces'):
        v, f = mesh.vertices, mesh.faces
    elif hasattr(mesh, 'keys') and 'verts' in mesh and 'faces' in mesh:
        v, f = mesh['verts'], mesh['faces']
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        v, f = mesh
    else:
        raise TypeError(f'{who}: expected .vertices / .faces, verts / faces keys, a (verts, faces) pair or a path, got {type(mesh).__name__}')
    v, f = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v), torch.as_tensor(np.asarray(f) if not isinstance(f, torch.Tensor) else f)
    if v.ndim == 3 and v.shape[0] == 1:
        v = v[0]
    if f.ndim == 3 and f.shape[0] == 1:
        f = f[0]
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f'{who}: verts must be (V,3) and faces (F,3), got {tuple(v.shape)} and {tuple(f.shape)}')
    return v, f


def mean_distance(mesh, points) -> torch.Tensor:
    """the mean over points (n,3) of their distance to a built mesh (Engine.mesh): sqrt(d2) in double, a 0-d float64 device tensor"""
    return mesh.closest(points, want=('d2',)).d2.double().sqrt().mean()


def chamfer_and_p2s(src_mesh, tgt_mesh, src_pts, tgt_pts, p2s_pts, out=None) -> torch.Tensor:
    """the arithmetic of the two metrics on explicit sample points (mesh_evaluator.py:71-82, 91-96): src_pts / p2s_pts lie on the source
    surface, tgt_pts on the target's; src_mesh / tgt_mesh are built meshes.  Returns (or fills) a float64 (2,) device tensor
    [chamfer, p2s]; nothing is read back."""
    src_tgt, tgt_src = mean_distance(tgt_mesh, src_pts), mean_distance(src_mesh, tgt_pts)
    res = torch.stack([(src_tgt + tgt_src) / 2, mean_distance(tgt_mesh, p2s_pts)])
    if out is None:
        return res
    out.copy_(res)
    return out


class MeshEvaluator:
    """lib/evaluators/mesh_evaluator.py:36-98 on the device.  engine: the Engine that owns the HIP context (default: Evaluator.engine)."""

    def __init__(self, engine=None, generator=None):
        self.engine, self.generator = engine, generator
        self._src = self._tgt = None          # (verts, faces, built mesh)

    def _eng(self):
        eng = self.engine or Evaluator.engine
        if eng is None:
            raise RuntimeError('MeshEvaluator needs the engine that owns the HIP context (Evaluator.engine = net.engine()); no CPU fallback')
        return eng

    def _set(self, mesh, who):
        eng = self._eng()
        v, f = _as_mesh(mesh, who)
        v = v.to(eng.device, torch.float32)
        return v, f.to(eng.device), eng.mesh(v, f)       # the build takes the faces where they are (host faces stay on the host); the sampling a device copy

    def set_src_mesh(self, mesh):
        self._src = self._set(mesh, 'set_src_mesh')

    def set_tgt_mesh(self, tgt):
        self._tgt = self._set(tgt, 'set_tgt_mesh')

    def _sample(self, which, count):
        return mesh_utils.sample_surface(which[0], which[1], count, self.generator)[0]

    def get_chamfer_dist(self, num_samples=1000) -> torch.Tensor:
        src_pts = self._sample(self._src, num_samples)
        tgt_pts = self._sample(self._tgt, num_samples)
        return (mean_distance(self._tgt[2], src_pts) + mean_distance(self._src[2], tgt_pts)) / 2

    def get_surface_dist(self, num_samples=10000) -> torch.Tensor:
        return mean_distance(self._tgt[2], self._sample(self._src, num_samples))

    def close(self):
        for m in (self._src, self._tgt):
            if m is not None:
                m[2].close()
        self._src = self._tgt = None


class Evaluator:
    engine = None      # the Engine that owns the HIP context (set once: Evaluator.engine = net.engine())
    GROW = 64          # rows the table grows by

    def __init__(self, generator=None):
        self.metrics = None      # the per-frame lists of the last summary
        self.generator = generator
        self._table = None
        self._n = 0

    def __len__(self):
        return self._n

    def _row(self, dev):
        if self._table is None or self._n == self._table.shape[0]:
            grown = torch.empty(self._n + self.GROW, 2, dtype=torch.float64, device=dev)
            if self._n:
                grown[:self._n].copy_(self._table)          # on the stream, behind the calls that filled it
            self._table = grown
        self._n += 1
        return self._table[self._n - 1]

    def evaluate(self, output, batch, engine=None, generator=None):
        eng = engine or Evaluator.engine
        if eng is None:
            raise RuntimeError('Evaluator.evaluate needs the engine of the network (Evaluator.engine = net.engine()); no CPU fallback')
        ev = MeshEvaluator(eng, generator if generator is not None else self.generator)
        try:
            ev.set_src_mesh(output['mesh'])
            ev.set_tgt_mesh(batch['obj'][0])
            row = self._row(eng.device)
            row[0] = ev.get_chamfer_dist()
            row[1] = ev.get_surface_dist()
        finally:
            ev.close()

    def summarize(self):
        if self._n == 0:
            raise RuntimeError('Evaluator.summarize: no frame was evaluated')
        rows = self._table[:self._n].cpu().numpy()            # the one device-to-host copy
        self.metrics = {'chamfer': rows[:, 0].tolist(), 'p2s': rows[:, 1].tolist()}      # the reference's chamfer.npy / p2s.npy
        self._table, self._n = None, 0
        return {k: float(np.mean(v)) for k, v in self.metrics.items()}

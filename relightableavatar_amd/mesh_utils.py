"""Mesh helpers around the device's exact closest-point query (Engine.mesh, include/relightableavatar.h: ra_mesh_closest).

    bvh_distance(pts, verts, faces)                                   lib/utils/mesh_utils.py:758-764
    sample_closest_points_on_surface(points, verts, faces, values)    lib/utils/sample_utils.py:681-724
    sample_blend_K_closest_points(src, ref, values, K)                lib/utils/sample_utils.py:631-646 (cast_knn_points :605-611)
    sample_surface(verts, faces, count, generator)                    trimesh.sample.sample_surface's method
    load_obj(path)                                                    what trimesh.load gives the mesh evaluator: vertices and faces

The two distance functions take the engine that owns the HIP context (engine=, default: evaluators.mesh_evaluator.Evaluator.engine); they
have no CPU fallback.  sample_blend_K_closest_points, sample_surface and load_obj are plain torch / text and run anywhere.  Batches: the reference's signatures carry a
batch dimension; B == 1 is supported, B > 1 is refused.
"""
import torch


def _engine(engine):
    if engine is None:
        from .evaluators import mesh_evaluator
        engine = mesh_evaluator.Evaluator.engine
    if engine is None:
        raise RuntimeError('mesh_utils: needs the engine that owns the HIP context (engine=, or Evaluator.engine = net.engine()); no CPU fallback')
    return engine


def bvh_distance(pts: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, engine=None) -> torch.Tensor:
    """pts (N,3), verts (V,3), faces (F,3) -> (N,) the plain (not squared) distance of every point to the mesh, |pts - closest| as the
    reference computes it from bvh_distance_queries' closest points."""
    if pts.ndim != 2 or verts.ndim != 2 or faces.ndim != 2:
        raise ValueError('bvh_distance: pts (N,3), verts (V,3), faces (F,3) — the reference adds the batch dimension itself')
    mesh = _engine(engine).mesh(verts, faces)
    try:
        return mesh.closest(pts, want=('d2',)).d2.sqrt()
    finally:
        mesh.close()


def sample_closest_points_on_surface(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, values: torch.Tensor = None, engine=None):
    """points (1,N,3), verts (1,V,3), faces (1,F,3), values (1,V,D) or None.  Without values: the distances (1,N,1); with values:
    (interpolated values (1,N,D), distances (1,N,1)).

    The distance is the PLAIN one, not the squared one: the reference's point_mesh_distance wrapper (sample_utils.py:265-307) takes the
    square root of pytorch3d's squared point-to-face distance.
    The values are interpolated with the barycentrics of the CLOSEST POINT in its face.  The reference takes those of the query point's
    projection onto the face's plane (points_to_barycentric, :432-445), which may lie outside the face and then extrapolates; the two
    agree wherever the closest point is interior to the face."""
    if points.ndim != 3 or verts.ndim != 3 or faces.ndim != 3:
        raise ValueError('sample_closest_points_on_surface: points (B,N,3), verts (B,V,3), faces (B,F,3)')
    if points.shape[0] != 1 or verts.shape[0] != 1 or faces.shape[0] != 1:
        raise NotImplementedError('sample_closest_points_on_surface: batches with B > 1 are not supported')
    n = points.shape[1]
    mesh = _engine(engine).mesh(verts[0], faces[0])
    try:
        if values is None:
            return mesh.closest(points[0], want=('d2',)).d2.sqrt().view(1, n, 1)
        out = mesh.closest(points[0], want=('d2', 'face', 'bary'))
    finally:
        mesh.close()
    values = values.reshape(-1, values.shape[-1]).to(out.bary.device)
    corners = faces[0].to(out.bary.device).long()[out.face.long().clamp_min(0)]       # (N,3); face -1 (a non-finite point) has NaN barycentrics
    interp = (values[corners] * out.bary[..., None].to(values.dtype)).sum(1)
    return interp.view(1, n, -1), out.d2.sqrt().view(1, n, 1)


def sample_blend_K_closest_points(src: torch.Tensor, ref: torch.Tensor, values: torch.Tensor = None, K: int = 4, eps: float = 1e-8, chunk: int = 8192):
    """src (1,N,3), ref (1,V,3), values (1,V,D) or None.  The exact K nearest points of ref per point of src (squared distances as
    sum((p - v)^2), like pytorch3d's knn_points), their PLAIN distances d_k (the reference takes the square root first), weights
    w_k = 1 / (d_k + eps) normalised to sum 1.  Without values: sum w_k d_k as (1,N,1); with values: (sum w_k values[k] (1,N,D), that
    (1,N,1)).  Plain torch on src's device, in chunks of rows."""
    if src.ndim != 3 or ref.ndim != 3:
        raise ValueError('sample_blend_K_closest_points: src (B,N,3), ref (B,V,3)')
    if src.shape[0] != 1 or ref.shape[0] != 1:
        raise NotImplementedError('sample_blend_K_closest_points: batches with B > 1 are not supported')
    p, v = src[0].float(), ref[0].float().to(src.device)
    n = p.shape[0]
    d2s, idxs = [], []
    for i in range(0, max(n, 1), chunk):
        q = p[i:i + chunk]
        d2 = ((q[:, None, :] - v[None, :, :]) ** 2).sum(-1)
        top = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
        d2s.append(top.values)
        idxs.append(top.indices)
    dists, idx = torch.cat(d2s).sqrt(), torch.cat(idxs)
    w = 1 / (dists + eps)
    w = w / w.sum(dim=-1, keepdim=True)
    blended = (dists * w).sum(-1).view(1, n, 1)
    if values is None:
        return blended
    values = values.reshape(-1, values.shape[-1]).to(src.device)
    return torch.einsum('nkd,nk->nd', values[idx], w.to(values.dtype)).view(1, n, -1), blended


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, count: int, generator: torch.Generator = None):
    """count points uniformly distributed over the surface, and the face of each: trimesh.sample.sample_surface's method.  The face is
    drawn through the cumulative face area in float64 and searchsorted; the point is origin + r0 e0 + r1 e1 with two uniform lengths
    that are reflected (r -> 1 - r, both) where their sum exceeds 1.  Device-agnostic torch: runs where verts lives; the generator
    must live on that device.  Returns (points (count,3) in verts' dtype, face ids (count,) int64)."""
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError('sample_surface: verts (V,3), faces (F,3)')
    dev = verts.device
    faces = faces.to(dev).long()
    tri = verts[faces].double()                                            # (F,3,3)
    e0, e1 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = torch.linalg.cross(e0, e1).norm(dim=-1) * 0.5
    cum = torch.cumsum(area, 0)
    pick = torch.rand(count, dtype=torch.float64, device=dev, generator=generator) * cum[-1]
    fid = torch.searchsorted(cum, pick).clamp_max(faces.shape[0] - 1)
    r = torch.rand(count, 2, dtype=torch.float64, device=dev, generator=generator)
    r = torch.where(r.sum(1, keepdim=True) > 1.0, 1.0 - r, r)
    pts = tri[fid, 0] + r[:, :1] * e0[fid] + r[:, 1:] * e1[fid]
    return pts.to(verts.dtype), fid


def load_obj(path):
    """the `v` and `f` records of a Wavefront OBJ -> (verts (V,3) float32, faces (F,3) int64, zero-based).  Triangles only; the
    index forms a, a/b, a//c and a/b/c are accepted (the vertex index is the first field).
    Every other record type is skipped (vn, vt, o, g, s, usemtl, mtllib, comments); a face that is not a triangle, a vertex without
    three coordinates or an index outside the vertices (a relative, negative one too) is refused."""
    verts, faces = [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            tok = line.split()
            if not tok or tok[0] not in ('v', 'f'):
                continue
            if tok[0] == 'v':
                if len(tok) < 4:
                    raise ValueError(f'{path}:{no}: a vertex needs three coordinates')
                verts.append([float(t) for t in tok[1:4]])
            else:
                if len(tok) != 4:
                    raise ValueError(f'{path}:{no}: only triangles are supported, this face has {len(tok) - 1} corners')
                faces.append([int(t.split('/')[0]) for t in tok[1:]])
    if not verts or not faces:
        raise ValueError(f'{path}: no vertices or no faces')
    v = torch.tensor(verts, dtype=torch.float32)
    f = torch.tensor(faces, dtype=torch.int64)
    f = f - 1
    if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
        raise ValueError(f'{path}: a face index lies outside the {v.shape[0]} vertices')
    return v, f

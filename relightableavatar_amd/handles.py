"""Mesh, Topology, Cloth: the handles an Engine's context owns (ra_mesh, ra_topo, ra_cloth of the C ABI), with one lifecycle."""
import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import check
from .base_utils import dotdict


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _i32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.int32).contiguous()


def _want(who, want, allowed):
    want = tuple(want)
    if not want or any(k not in allowed for k in want):
        raise ValueError(f'{who}: want must be a non-empty subset of {allowed}')
    return want


class Handle:
    """what Mesh, Topology and Cloth share: a handle of the engine's context and a weak reference to the engine.  close() — or garbage
    collection — releases the handle while the engine lives; once the engine is gone the context has freed it and it only refuses."""
    _NOUN, _DESTROY = 'handle', None        # the noun of the two messages, the library's destroy entry

    def __init__(self, engine, handle):
        self._engine, self._handle = weakref.ref(engine), handle

    def _live_engine(self):
        eng = self._engine()
        if eng is None or not eng.ctx.value:
            raise _lib.RaError(f'{self._NOUN.capitalize()}: the engine that built this {self._NOUN} is gone')
        if not self._handle.value:
            raise _lib.RaError(f'{self._NOUN.capitalize()}: closed')
        return eng

    def close(self):
        eng = self._engine()
        if self._handle.value and eng is not None and eng.ctx.value:
            check(getattr(eng.lib, self._DESTROY)(eng.ctx, self._handle), self._DESTROY)
        self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_closest_backward_args(points, out, g_d2, g_attr, want):
    """the argument errors of mesh_closest_backward, raised before any context is touched -> (want, n, C)"""
    want = _want('closest_backward', want, Mesh.GRAD_WANT)
    if any(k not in out for k in ('closest', 'face', 'bary')):
        raise ValueError("closest_backward: out must hold the forward's closest, face and bary")
    if g_d2 is None and ('dpts' in want or 'dverts' in want):
        raise ValueError('closest_backward: dpts and dverts need g_d2')
    if g_attr is None and 'dattr' in want:
        raise ValueError('closest_backward: dattr needs g_attr')
    n = points.reshape(-1, 3).shape[0]
    if tuple(out['closest'].shape) != (n, 3) or tuple(out['bary'].shape) != (n, 3) or tuple(out['face'].shape) != (n,):
        raise ValueError(f'closest_backward: out.closest and out.bary must be ({n}, 3) and out.face ({n},)')
    if g_d2 is not None and g_d2.numel() != n:
        raise ValueError(f'closest_backward: g_d2 must hold {n} values')
    Cn = 0
    if g_attr is not None:
        if g_attr.ndim != 2 or g_attr.shape[0] != n or g_attr.shape[1] > 64:
            raise ValueError(f'closest_backward: g_attr must be ({n}, C) with C <= 64')
        Cn = g_attr.shape[1]
    return want, n, Cn


class Mesh(Handle):
    """a triangle mesh built for closest-point queries (Engine.mesh).  It belongs to its engine's context: close() — or garbage
    collection — releases it while the engine lives; once the engine is gone the context has freed it and the handle only refuses."""
    _NOUN, _DESTROY = 'mesh', 'ra_mesh_destroy'
    WANT = ('d2', 'closest', 'face', 'bary')

    GRAD_WANT = ('dpts', 'dverts', 'dattr')

    def __init__(self, engine, handle, n_faces, faces_dev=None, n_verts=None):
        super().__init__(engine, handle)
        # (F,3) int32 and V: what closest_backward reads.  Host faces go to the device at the first backward and stay there
        self.n_faces, self._faces, self.n_verts = n_faces, faces_dev, n_verts

    def closest(self, points, want=WANT, brute=False, sort=True):
        """points (n,3) -> dotdict of the wanted outputs on the device, all fp32 but face (int32): d2 (n,) squared distance, closest
        (n,3), face (n,) original index of a face that attains d2 (the lowest among equals), bary (n,3) of closest in that face.
        brute: scan every face (the same bits, slower).  sort=False: do not Morton-sort the points internally (the same bits;
        measurement).  A non-finite point: NaN and face -1.  Nothing is read back."""
        eng = self._live_engine()
        want = _want('Mesh.closest', want, self.WANT)
        d = eng.device
        pts = _f32(points.reshape(-1, 3), d)
        n = pts.shape[0]
        out = dotdict()
        for k in want:
            out[k] = torch.empty((n,) if k in ('d2', 'face') else (n, 3), dtype=torch.int32 if k == 'face' else torch.float32, device=d)
        flags = (_lib.RA_MESH_BRUTE if brute else 0) | (0 if sort else _lib.RA_MESH_UNSORTED)
        check(eng.lib.ra_mesh_closest(eng.ctx, self._handle, _ptr(pts), n, flags, *[_ptr(out.get(k)) for k in self.WANT], eng.stream), 'ra_mesh_closest')
        return out

    def faces_device(self):
        """the mesh's (F,3) int32 faces on the engine's device; uploaded at the first call"""
        eng = self._live_engine()
        if self._faces is None or self.n_verts is None:
            raise _lib.RaError('Mesh: made without its faces (build it with Engine.mesh)')
        if self._faces.device != eng.device:
            self._faces = self._faces.to(eng.device)
        return self._faces

    def closest_backward(self, points, out, g_d2=None, g_attr=None, want=GRAD_WANT):
        """The backward of closest (include/relightableavatar.h: ra_mesh_closest_backward).  points (n,3); out: the dotdict closest
        returned, with closest, face and bary; g_d2 (n,) the upstream gradient of d2, the SQUARED distance; g_attr (n,C), 0 <= C <= 64,
        the upstream gradient of C attribute channels interpolated at the closest point -> dotdict of the wanted outputs, float32 on
        the device: dpts (n,3), dverts (V,3), dattr (V,C).  dpts and dverts need g_d2, dattr needs g_attr; a wanted output whose
        upstream gradient is missing is refused.  A row whose face is -1 (a non-finite point) contributes nothing and gets dpts 0.
        No float atomics: the same inputs give the same bits, whichever outputs are asked for.  Nothing is read back."""
        check_closest_backward_args(points, out, g_d2, g_attr, want)
        return self._live_engine().mesh_closest_backward(self.faces_device(), self.n_verts, points, out, g_d2, g_attr, want)

    @staticmethod
    def _winding_flags(who, shape):
        if shape not in (None, 'one_pass', 'split'):
            raise ValueError(f"{who}: shape must be None, 'one_pass' or 'split'")
        return {None: 0, 'one_pass': _lib.RA_WINDING_ONE_PASS, 'split': _lib.RA_WINDING_SPLIT}[shape]

    def winding(self, points, shape=None):
        """points (n,3) -> (n,) float32 on the device: the generalised winding number of the mesh at every point (include/
        relightableavatar.h: ra_mesh_winding), about 1 inside, 0 outside.  A function of (point, mesh) alone, bit for bit.  A non-finite
        point and a point on a vertex: NaN.  shape: None lets the library choose the launch, 'one_pass' / 'split' force one (the same
        bits; tests and measurement).  Nothing is read back."""
        eng = self._live_engine()
        flags = self._winding_flags('Mesh.winding', shape)
        pts = _f32(points.reshape(-1, 3), eng.device)
        n = pts.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=eng.device)
        check(eng.lib.ra_mesh_winding(eng.ctx, self._handle, _ptr(pts), n, flags, _ptr(out), eng.stream), 'ra_mesh_winding')
        return out

    def winding_grad(self, points, shape=None):
        """points (n,3) -> (winding (n,), grad (n,3)) float32 on the device: Mesh.winding's number, the same bits, and its gradient with
        respect to the point (include/relightableavatar.h: ra_mesh_winding_grad) — the gradient of the function Mesh.winding computes,
        in closed form.  A row is a function of (point, mesh) alone, bit for bit.  A non-finite point and a point on a vertex: NaN in
        both; a point on the segment of an edge: a NaN gradient.  shape: as Mesh.winding's.  Nothing is read back."""
        eng = self._live_engine()
        flags = self._winding_flags('Mesh.winding_grad', shape)
        pts = _f32(points.reshape(-1, 3), eng.device)
        n = pts.shape[0]
        w = torch.empty(n, dtype=torch.float32, device=eng.device)
        grad = torch.empty((n, 3), dtype=torch.float32, device=eng.device)
        check(eng.lib.ra_mesh_winding_grad(eng.ctx, self._handle, _ptr(pts), n, flags, _ptr(w), _ptr(grad), eng.stream), 'ra_mesh_winding_grad')
        return w, grad

    RAY_WANT = ('t', 'face', 'uv', 'count')

    def raycast(self, ray_o, ray_d, want=RAY_WANT, brute=False, sort=True):
        """ray_o, ray_d (n,3) -> dotdict of the wanted outputs on the device (include/relightableavatar.h: ra_mesh_raycast): t (n,)
        fp32 the nearest hit in units of |ray_d| (+inf without one), face (n,) int32 the original index of the face hit (the lowest
        among equal t; -1), uv (n,2) fp32 its barycentrics of b and c (NaN), count (n,) int32 the number of faces the ray meets (its
        parity is the reference's ray_stabbing).  With count wanted nothing is pruned by t: ask for it only where it is used.
        brute: test every face (the same bits, slower).  sort=False: do not re-order the rays internally (the same bits;
        measurement).  A non-finite ray: NaN, face -1, count -1.  Nothing is read back."""
        eng = self._live_engine()
        want = _want('Mesh.raycast', want, self.RAY_WANT)
        d = eng.device
        o, r = _f32(ray_o.reshape(-1, 3), d), _f32(ray_d.reshape(-1, 3), d)
        if o.shape != r.shape:
            raise ValueError('Mesh.raycast: ray_o and ray_d must hold the same number of rays')
        n = o.shape[0]
        out = dotdict()
        for k in want:
            out[k] = torch.empty((n, 2) if k == 'uv' else (n,), dtype=torch.int32 if k in ('face', 'count') else torch.float32, device=d)
        flags = (_lib.RA_RAYCAST_BRUTE if brute else 0) | (0 if sort else _lib.RA_RAYCAST_UNSORTED)
        check(eng.lib.ra_mesh_raycast(eng.ctx, self._handle, _ptr(o), _ptr(r), n, flags, *[_ptr(out.get(k)) for k in self.RAY_WANT], eng.stream), 'ra_mesh_raycast')
        return out

    def icp_residual(self, points, point_normals, face_normals, dist_th=0.1, angle_th=0.7071067811865476, want_grad=True, want_keep=False):
        """points, point_normals (n,3), face_normals (F,3) of THIS mesh in its original face order -> dotdict on the device
        (ra_icp_residual): sums (2,) float64 — the sum of |p - closest|^2 over the kept rows and their count; loss = sums[0] /
        sums[1], a float64 scalar (NaN when nothing is kept); grad (n,3) float32 = d loss / d points with the closest points held
        constant; keep (n,) bool.  Kept: squared distance < fl32(dist_th^2) and dot(face_normals[face], point_normals) > angle_th."""
        eng = self._live_engine()
        d = eng.device
        p, n0, n1 = _f32(points.reshape(-1, 3), d), _f32(point_normals.reshape(-1, 3), d), _f32(face_normals.reshape(-1, 3), d)
        n = p.shape[0]
        if n0.shape != p.shape or n1.shape[0] != self.n_faces:
            raise ValueError(f'Mesh.icp_residual: point_normals must be ({n}, 3) and face_normals ({self.n_faces}, 3)')
        out = dotdict(sums=torch.empty(2, dtype=torch.float64, device=d))
        if want_grad:
            out.grad = torch.zeros(n, 3, dtype=torch.float32, device=d)
        keep = torch.zeros(n, dtype=torch.uint8, device=d) if want_keep else None
        check(eng.lib.ra_icp_residual(eng.ctx, self._handle, _ptr(p) if n else None, _ptr(n0) if n else None, n, _ptr(n1) if n else None, float(dist_th),
                                      float(angle_th), _ptr(out.sums), _ptr(out.grad) if want_grad and n else None, _ptr(keep) if want_keep and n else None,
                                      eng.stream), 'ra_icp_residual')
        out.loss = out.sums[0] / out.sums[1]
        if want_keep:
            out.keep = keep != 0
        return out


class Topology(Handle):
    """the connectivity of a triangle mesh on the device (Engine.topology; include/relightableavatar.h: ra_topo_create): unique
    edges, half-edges, vertex neighbours.  Immutable; holds no positions.  It belongs to its engine's context like a Mesh: close() — or
    garbage collection — releases it while the engine lives; once the engine is gone the handle only refuses.  Arrays come back as
    int64 tensors on the device, like the reference's, and are cached."""
    _NOUN, _DESTROY = 'topology', 'ra_topo_destroy'

    def __init__(self, engine, handle):
        super().__init__(engine, handle)
        self._cache = {}
        sizes = (C.c_int * 7)()
        check(engine.lib.ra_topo_sizes(engine.ctx, handle, sizes), 'ra_topo_sizes')
        self.F, self.V, self.E, self.max_valence, self.max_outgoing, self.readbacks, self.max_edge_count = (int(v) for v in sizes)
        self.HE = 3 * self.F

    def array(self, name, dtype=torch.int64):
        """one of _lib.RA_TOPO_ARRAYS as a device tensor (int32 is what the library holds; int64 is a cast)"""
        key = (name, dtype)
        if key not in self._cache:
            eng = self._live_engine()
            n = {'vert': self.HE, 'twin': self.HE, 'edge': self.HE, 'edges': 2 * self.E, 'edge_counts': self.E, 'edge_he_start': self.E + 1,
                 'edge_he': self.HE, 'nbr_start': self.V + 1, 'nbr': 2 * self.E, 'out_start': self.V + 1, 'out_he': self.HE}[name]
            out = torch.empty(n, dtype=torch.int32, device=eng.device)
            check(eng.lib.ra_topo_array(eng.ctx, self._handle, _lib.RA_TOPO_ARRAYS.index(name), _ptr(out) if n else None, eng.stream), 'ra_topo_array')
            self._cache[key] = out.to(dtype)
        return self._cache[key]

    @property
    def edges(self):
        """(E,2) the true (min, max) of every edge, lexicographic"""
        return self.array('edges').view(-1, 2)

    @property
    def edge_counts(self):
        """(E,) half-edges per edge: 2 manifold, 1 boundary"""
        return self.array('edge_counts')

    @property
    def halfedge(self):
        """the reference's triangle_to_halfedge structure without positions: twin, vert, edge (HE,), HE, E, F, V"""
        return dotdict(verts=None, twin=self.array('twin'), vert=self.array('vert'), edge=self.array('edge'), HE=self.HE, E=self.E, F=self.F, V=self.V)

    def face_connectivity(self):
        """the reference's get_face_connectivity: (edges_connecting_faces (M,2), connected_faces (M,2)) over the M manifold edges in
        edge order; within an edge the lower half-edge comes first (the reference leaves that order to an unstable argsort)."""
        start, he = self.array('edge_he_start'), self.array('edge_he')
        first = start[:-1][self.edge_counts == 2]
        inds = torch.stack([he[first], he[first + 1]], dim=1) if first.numel() else torch.zeros(0, 2, dtype=torch.int64, device=he.device)
        return self.array('vert')[inds], inds // 3

    def smooth(self, values, inds=None, alpha=0.33, iter=90):
        """Taubin smoothing of values (V,C) or (V,), 1 <= C <= 64 -> a new float32 tensor on the device (ra_mesh_smooth): the
        reference's laplacian_smoothing on this topology's edges.  inds: integer indices or a bool mask of the rows that move."""
        eng = self._live_engine()
        v = _f32(values, eng.device)
        if v.shape[:1] != (self.V,) or v.ndim > 2:
            raise ValueError(f'Topology.smooth: values must be ({self.V}, C) or ({self.V},)')
        if self.V == 0:
            return v.clone()
        v2 = v.reshape(self.V, -1)
        out = torch.empty_like(v2)
        ind = None
        if inds is not None:
            ind = torch.as_tensor(inds, device=eng.device)
            ind = ind.nonzero(as_tuple=True)[0] if ind.dtype == torch.bool else ind.reshape(-1).to(torch.int64)
            ind = torch.where(ind < 0, ind + self.V, ind).contiguous()
        check(eng.lib.ra_mesh_smooth(eng.ctx, self._handle, _ptr(v2), self.V, v2.shape[1], _ptr(ind) if ind is not None and ind.numel() else None,
                                     0 if ind is None else ind.numel(), float(alpha), int(iter), _ptr(out), eng.stream), 'ra_mesh_smooth')
        if ind is not None and ind.numel() == 0:       # an empty selection moves nothing (a NULL list would move everything)
            out.copy_(v2)
        return out.reshape(v.shape)

    def subdivide(self, values):
        """one Loop subdivision step of values (V,C), 1 <= C <= 64 -> (values (V + E, C) float32, faces (4F, 3) int32, Topology of the
        subdivided mesh), all on the device (ra_mesh_subdivide): the reference's halfedge_loop_subdivision.  Row V + e is the new
        vertex of edge e.  The child comes from index arithmetic: nothing is sorted or read back."""
        eng = self._live_engine()
        v = _f32(values, eng.device)
        if v.ndim != 2 or v.shape[0] != self.V or not 1 <= v.shape[1] <= 64:
            raise ValueError(f'Topology.subdivide: values must be ({self.V}, C) with 1 <= C <= 64')
        out = torch.empty(self.V + self.E, v.shape[1], dtype=torch.float32, device=eng.device)
        faces = torch.empty(4 * self.F, 3, dtype=torch.int32, device=eng.device)
        child = C.c_void_p()
        check(eng.lib.ra_mesh_subdivide(eng.ctx, self._handle, _ptr(v) if v.numel() else None, self.V, v.shape[1], _ptr(out) if out.numel() else None,
                                        _ptr(faces) if self.F else None, C.byref(child), eng.stream), 'ra_mesh_subdivide')
        return out, faces, Topology(eng, child)

    def dilate(self, mask, steps):
        """mask (V,) bool -> bool: the vertex-mask dilation of the reference's segment_mesh, (A^steps mask) != 0; steps < 0 dilates
        the complement, as there (ra_topo_dilate)."""
        eng = self._live_engine()
        m = torch.as_tensor(mask, device=eng.device).reshape(-1) != 0
        if m.shape[0] != self.V:
            raise ValueError(f'Topology.dilate: mask must hold {self.V} entries')
        steps = int(steps)
        if steps < 0:
            m = ~m
        src = m.to(torch.uint8).contiguous()
        out = torch.empty_like(src)
        check(eng.lib.ra_topo_dilate(eng.ctx, self._handle, _ptr(src), self.V, abs(steps), _ptr(out), eng.stream), 'ra_topo_dilate')
        out = out != 0
        return ~out if steps < 0 else out

    def _rows(self, who, x, eng):
        v = _f32(x, eng.device)
        if v.shape[:1] != (self.V,) or v.ndim not in (1, 2) or (v.ndim == 2 and not 1 <= v.shape[1] <= 64):
            raise ValueError(f'Topology.{who}: rows must be ({self.V}, C) with 1 <= C <= 64, or ({self.V},)')
        return v, v.reshape(self.V, 1 if v.ndim == 1 else v.shape[1])

    def diffuse_apply(self, x, lam):
        """x (V,C) or (V,) -> M x as a new float32 tensor, M = I + lam L the large-steps operator on this topology's unique edges
        (ra_topo_diffuse_apply): largesteps' to_differential."""
        eng = self._live_engine()
        v, v2 = self._rows('diffuse_apply', x, eng)
        out = torch.empty_like(v2)
        check(eng.lib.ra_topo_diffuse_apply(eng.ctx, self._handle, _ptr(v2) if self.V else None, self.V, max(v2.shape[1], 1), float(lam),
                                            _ptr(out) if self.V else None, eng.stream), 'ra_topo_diffuse_apply')
        return out.reshape(v.shape)

    def diffuse_solve(self, b, lam, x0=None, tol=1e-9, max_iter=256, info=False):
        """b (V,C) or (V,) -> x with M x = b as a new float32 tensor (ra_topo_diffuse_solve): Jacobi-preconditioned conjugate
        gradients in float64, every channel its own system, stopped at |r| <= tol |b| or after max_iter iterations; x0 warm-starts
        it.  Nothing is read back.  info=True: (x, dotdict(iters (C,) int32, stop (C,) int32, residual (C,) float64)) on the device."""
        eng = self._live_engine()
        v, v2 = self._rows('diffuse_solve', b, eng)
        start = None
        if x0 is not None:
            start = _f32(x0, eng.device).reshape(self.V, -1)
            if start.shape != v2.shape:
                raise ValueError('Topology.diffuse_solve: x0 must have the shape of b')
        out = torch.empty_like(v2)
        Cn = max(v2.shape[1], 1)
        rec = torch.zeros(Cn, 2, dtype=torch.float64, device=eng.device) if info else None
        check(eng.lib.ra_topo_diffuse_solve(eng.ctx, self._handle, _ptr(v2) if self.V else None, self.V, Cn, float(lam),
                                            _ptr(start) if start is not None and self.V else None, float(tol), int(max_iter),
                                            _ptr(out) if self.V else None, _ptr(rec), eng.stream), 'ra_topo_diffuse_solve')
        out = out.reshape(v.shape)
        if not info:
            return out
        words = rec[:, 0].contiguous().view(torch.int32).view(Cn, 2)
        return out, dotdict(iters=words[:, 0], stop=words[:, 1], residual=rec[:, 1])

    NORMALS = ('face_normal', 'face_area', 'vert_normal')

    def normals(self, verts, want=NORMALS):
        """verts (V,3) -> dotdict of the wanted float32 outputs on the device (ra_mesh_normals): face_normal (F,3) the reference's
        face_normals, face_area (F,) its get_face_areas, vert_normal (V,3) the area-weighted vertex normals of pytorch3d."""
        eng = self._live_engine()
        want = _want('Topology.normals', want, self.NORMALS)
        v = _f32(verts, eng.device)
        if v.shape != (self.V, 3):
            raise ValueError(f'Topology.normals: verts must be ({self.V}, 3)')
        out = dotdict()
        for k in want:
            out[k] = torch.zeros({'face_normal': (self.F, 3), 'face_area': (self.F,), 'vert_normal': (self.V, 3)}[k], dtype=torch.float32, device=eng.device)
        ptrs = [_ptr(out[k]) if k in out and out[k].numel() else None for k in self.NORMALS]
        if any(p is not None for p in ptrs):      # an empty output has no address
            check(eng.lib.ra_mesh_normals(eng.ctx, self._handle, _ptr(v), self.V, *ptrs, eng.stream), 'ra_mesh_normals')
        return out


class Cloth(Handle):
    """a garment on a Topology (Engine.cloth; include/relightableavatar.h: ra_cloth_create): rest areas, Dm_inv, vertex masses and the
    hinges of the manifold edges, immutable, on the device.  It keeps its Topology alive.  close() — or garbage collection — releases
    it while the engine lives."""
    _NOUN, _DESTROY = 'cloth', 'ra_cloth_destroy'

    TERMS = {'stretch': _lib.RA_CLOTH_STRETCH, 'bending': _lib.RA_CLOTH_BENDING, 'gravity': _lib.RA_CLOTH_GRAVITY}

    def __init__(self, engine, handle, topology, coeffs):
        super().__init__(engine, handle)
        self.topology, self._cache = topology, None
        self.coeffs = coeffs        # A, stretch_coeff, bending_coeff, lame_mu, lame_lambda as the library derived them (float64)

    @property
    def arrays(self):
        """dotdict on the device: f_area (F,), Dm and Dm_inv (F,2,2), v_mass and inv_mass (V,) float32; f_connectivity and
        f_connectivity_edges (H,2) int64, the hinges in the order of Topology.face_connectivity().  The library keeps hinges per
        edge; dropping the edges without one is a masked copy here (it waits for the device once), then cached."""
        if self._cache is None:
            eng, t = self._live_engine(), self.topology
            out = dotdict()
            for k, (name, n, dt) in enumerate((('f_area', t.F, torch.float32), ('Dm', 4 * t.F, torch.float32), ('Dm_inv', 4 * t.F, torch.float32),
                                               ('v_mass', t.V, torch.float32), ('inv_mass', t.V, torch.float32), ('hinge_faces', 2 * t.E, torch.int32),
                                               ('hinge_verts', 2 * t.E, torch.int32))):
                a = torch.empty(n, dtype=dt, device=eng.device)
                check(eng.lib.ra_cloth_array(eng.ctx, self._handle, k, _ptr(a) if n else None, eng.stream), 'ra_cloth_array')
                out[name] = a
            out.Dm, out.Dm_inv = out.Dm.view(-1, 2, 2), out.Dm_inv.view(-1, 2, 2)
            hf, hv = out.pop('hinge_faces').view(-1, 2).long(), out.pop('hinge_verts').view(-1, 2).long()
            keep = hf[:, 0] >= 0
            out.f_connectivity, out.f_connectivity_edges = hf[keep], hv[keep]
            self._cache = out
        return self._cache

    def energy(self, x, terms=('stretch', 'bending'), gravity=9.81, grad=True):
        """x (B,V,3) -> (energy (B,3) float64: the per-row stretch, bending and gravity sums, 0 where a term is not selected; grad
        (B,V,3) float32 of the selected terms' sum, or None) on the device (ra_cloth_energy).  Not divided by B.  Asynchronous."""
        eng = self._live_engine()
        v = _f32(x, eng.device)
        if v.ndim != 3 or v.shape[1:] != (self.topology.V, 3) or v.shape[0] < 1:
            raise ValueError(f'Cloth.energy: x must be (B, {self.topology.V}, 3) with B >= 1')
        bits = 0
        for k in terms:
            bits |= self.TERMS[k]
        energy = torch.empty(v.shape[0], 3, dtype=torch.float64, device=eng.device)
        g = torch.empty_like(v) if grad else None
        check(eng.lib.ra_cloth_energy(eng.ctx, self._handle, _ptr(v) if v.numel() else None, v.shape[0], bits, float(gravity), _ptr(energy),
                                      _ptr(g) if g is not None and g.numel() else None, eng.stream), 'ra_cloth_energy')
        return energy, g

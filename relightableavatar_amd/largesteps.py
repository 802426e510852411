"""The large-steps parameterisation and optimiser that the reference's mesh fitting imports from the `largesteps` package
(lib/utils/mesh_utils.py:310-312), on the device (include/relightableavatar.h: ra_topo_diffuse_apply / _solve, ra_adam_uniform_step).

    compute_matrix(verts, faces, lambda_)          largesteps.geometry: M = I + lambda L, L the combinatorial Laplacian of the unique edges
    to_differential(M, v)                          largesteps.parameterize: u = M v
    from_differential(M, u, method='Cholesky')     v = M^-1 u; its gradient is M^-1 g, M being symmetric
    AdamUniform(params, lr=0.1, betas=(0.9, 0.999))    largesteps.optimize: Adam with ONE second-moment scalar per tensor

The package solves with a sparse Cholesky factorisation; here the solve is conjugate gradients in float64 on a Topology's neighbour
lists, stopped at a relative residual of 1e-9 — below float32's resolution of the answer.  `method` is checked
and does not change the algorithm.  No CPU fallback: a Matrix belongs to the engine that built its topology.
"""
import torch

from .mesh_utils import _engine

METHODS = ('Cholesky', 'CG')


class Matrix:
    """M = I + lambda L of one mesh: a Topology and lambda.  tol / max_iter are the solve's stopping rule."""

    def __init__(self, topology, lambda_, tol=1e-9, max_iter=256):
        self.topology, self.lambda_, self.tol, self.max_iter = topology, float(lambda_), float(tol), int(max_iter)

    def apply(self, x):
        return self.topology.diffuse_apply(x, self.lambda_)

    def solve(self, b, x0=None):
        return self.topology.diffuse_solve(b, self.lambda_, x0=x0, tol=self.tol, max_iter=self.max_iter)


def compute_matrix(verts: torch.Tensor, faces: torch.Tensor, lambda_: float, engine=None, tol=1e-9, max_iter=256) -> Matrix:
    """verts (V,3) — only their count is used — faces (F,3) integers, lambda_ >= 0 -> Matrix"""
    if verts.ndim != 2 or faces.ndim != 2 or faces.shape[-1] != 3:
        raise ValueError('compute_matrix: verts (V,3), faces (F,3)')
    return Matrix(_engine(engine).topology(faces, verts.shape[0]), lambda_, tol, max_iter)


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, v):
        ctx.M = M
        return M.apply(v)

    @staticmethod
    def backward(ctx, g):
        return None, ctx.M.apply(g.contiguous())


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, u, x0):
        ctx.M = M
        return M.solve(u, x0)

    @staticmethod
    def backward(ctx, g):
        return None, ctx.M.solve(g.contiguous()), None


def to_differential(M: Matrix, v: torch.Tensor) -> torch.Tensor:
    """u = M v, differentiable in v (the backward is the same product)"""
    return _Apply.apply(M, v)


def from_differential(M: Matrix, u: torch.Tensor, method: str = 'Cholesky', x0: torch.Tensor = None) -> torch.Tensor:
    """v = M^-1 u, differentiable in u (the backward is the same solve of the gradient).  x0 (no gradient) warm-starts the solve."""
    if method not in METHODS:
        raise ValueError(f'from_differential: method must be one of {METHODS}')
    return _Solve.apply(M, u, None if x0 is None else x0.detach())


class AdamUniform(torch.optim.Optimizer):
    """largesteps.optimize.AdamUniform: Adam whose second moment is ONE scalar per parameter tensor, the running maximum-square of the
    gradient, so that every coordinate takes the same step scale.  Parameters: contiguous float32 tensors on the engine's device."""

    def __init__(self, params, lr=0.1, betas=(0.9, 0.999), engine=None):
        super().__init__(params, dict(lr=lr, betas=betas))
        self._ra_engine = _engine(engine)

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['g1'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['g2'] = torch.zeros(1, dtype=torch.float32, device=p.device)
                state['step'] += 1
                self._ra_engine.adam_uniform_step(p.data, p.grad.contiguous(), state['g1'], state['g2'], state['step'], group['lr'], group['betas'])

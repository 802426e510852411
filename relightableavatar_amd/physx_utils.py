"""The reference's garment model (lib/utils/physx_utils.py) on the device: a Saint-Venant-Kirchhoff membrane, dihedral-angle bending,
gravity and the inertia terms — the SNUG losses — as autograd ops over the HIP library (include/relightableavatar.h: ra_cloth_create,
ra_cloth_energy, ra_cloth_inertia).  Names and signatures are the reference's.

    StVKMaterial(...), Garment(v, f, vm, fm, material)
    stretch_energy(v, garment), bending_energy(v, garment), gravity_energy(x, mass, g)        sum / B, differentiable in the positions
    cloth_energy(x, garment, stretch=True, bending=True, gravity=False)                    the selected terms in one launch sequence
    inertia_term, dynamic_term, inertia_term_sequence
    get_shape_matrix, deformation_gradient, green_strain_tensor                            small torch helpers, kept for callers

Everything numeric happens in the library, in fp32 element arithmetic with float64 sums; the 1 / B is applied here.  The gradient is
the library's analytic one (first order only: the ops are not twice differentiable).  No CPU fallback: a Garment belongs to the engine
that built it.  The XPBD variants (stretch_energy_constraints, bending_energy_constraints, xpbd_constraints) are stubs that raise:
the reference's own code has no working behaviour to be at parity with.
"""
import ctypes as C
from typing import Callable

import torch

from . import _lib
from .base_utils import dotdict
from .mesh_utils import _engine

XPBD_REASON = ('not built: in the reference xpbd_constraints raises a shape error whenever accum_lambda is left at its default (zeros_like(inv_mass) is '
               'B x F x 3 against an energy of B x F), bending_energy_constraints only runs at B = 1, and bending_energy_components is 0 / 0 on an '
               'exactly flat hinge — there is no working behaviour to be at parity with (DESIGN.md section 23)')


class StVKMaterial(dotdict):
    """the parameters of the StVK material model and, derived from them by the library in float64 (ra_cloth_material_derive, host
    only: csrc/ra_cloth_rules.hpp cloth_material), A, stretch_coeff, bending_coeff, lame_mu and lame_lambda — the ONE statement of those
    formulas, the same values ra_cloth_create rounds for its kernels"""

    DERIVED = ('A', 'stretch_coeff', 'bending_coeff', 'lame_mu', 'lame_lambda')

    def __init__(self, density=426 * 0.00047, thickness=0.00047, young_modulus=0.7e5, poisson_ratio=0.485, bending_multiplier=50.0,
                 stretch_multiplier=1.0, material_multiplier=1.0):
        given = dict(density=density, thickness=thickness, young_modulus=young_modulus, poisson_ratio=poisson_ratio,
                     bending_multiplier=bending_multiplier, stretch_multiplier=stretch_multiplier, material_multiplier=material_multiplier)
        self.update(given)
        record = _lib.ra_cloth_material(*[float(given[k]) for k, _ in _lib.CLOTH_MATERIAL_DEFAULTS])
        derived = (C.c_double * len(self.DERIVED))()
        _lib.check(_lib.lib().ra_cloth_material_derive(C.byref(record), derived), 'ra_cloth_material_derive')
        self.update(zip(self.DERIVED, derived))


class Garment(dotdict):
    """mesh and material of a garment, no batch dimension: v (V,3), f (F,3), vm (M,2) material coordinates, fm (F,3) into vm.  The
    attributes are the reference's — f_connectivity, f_connectivity_edges, f_connected_faces, f_area, v_mass, inv_mass, Dm, Dm_inv —
    as device tensors computed by the library; `cloth` is the Engine.cloth handle the energies run on."""

    def __init__(self, v: torch.Tensor, f: torch.Tensor, vm: torch.Tensor, fm: torch.Tensor, material: StVKMaterial = None, engine=None):
        eng = _engine(engine)
        self.material = material if material is not None else StVKMaterial()
        self.topology = eng.topology(f, v.shape[0])
        self.cloth = eng.cloth(self.topology, v, vm, fm, self.material)
        a = self.cloth.arrays
        self.f = f.to(eng.device).long()
        self.f_connectivity_edges, self.f_connectivity = a.f_connectivity_edges, a.f_connectivity
        self.f_connected_faces = self.f[self.f_connectivity.reshape(-1)].view(-1, 2, 3)
        self.f_area = a.f_area
        self.v = v
        self.v_mass, self.inv_mass = a.v_mass, a.inv_mass
        self.vm, self.fm = vm, fm
        self.Dm, self.Dm_inv = a.Dm, a.Dm_inv


# small torch helpers for callers; leading batch dimensions pass through
def get_shape_matrix(tris: torch.Tensor):
    """tris (..., 3, D) -> (..., D, 2): the two edges that run from the last corner to the first and to the second, as columns"""
    return (tris[..., :2, :] - tris[..., 2:, :]).transpose(-1, -2)


def deformation_gradient(tris: torch.Tensor, Dm_invs: torch.Tensor):
    """F = Ds Dm_inv of deformed triangles (..., 3, 3) against inverted material shape matrices (..., 2, 2)"""
    return torch.matmul(get_shape_matrix(tris), Dm_invs)


def green_strain_tensor(F: torch.Tensor) -> torch.Tensor:
    """G = (F^T F - 1) / 2"""
    gram = torch.matmul(F.transpose(-1, -2), F)
    return (gram - torch.eye(gram.shape[-1]).to(gram)) / 2


def _float32(who, *tensors):
    """the library's gradients are float32: another dtype would only fail later, inside autograd"""
    for t in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f'{who}: positions and velocities must be float32 tensors, got {t.dtype}')


class _Energy(torch.autograd.Function):
    """sum over the rows and the selected terms of ra_cloth_energy, / B; the backward scales the library's gradient"""

    @staticmethod
    def forward(ctx, x, cloth, terms, g):
        energy, grad = cloth.energy(x, terms=terms, gravity=g, grad=ctx.needs_input_grad[0])
        ctx.grad, ctx.B = grad, x.shape[0]
        ctx.mark_non_differentiable(energy)
        return (energy.sum() / x.shape[0]).to(torch.float32), energy

    @staticmethod
    def backward(ctx, d_total, _):
        return ctx.grad * (d_total / ctx.B).to(ctx.grad.dtype), None, None, None


def cloth_energy(x: torch.Tensor, garment: Garment, stretch=True, bending=True, gravity=False, g=9.81, per_term=False):
    """x (B,V,3) -> the sum of the selected energies / B (a float32 scalar, differentiable in x), from one launch sequence.
    per_term=True: (total, energy (B,3) float64 — the per-row stretch, bending and gravity sums, not divided, no gradient)"""
    terms = tuple(k for k, on in (('stretch', stretch), ('bending', bending), ('gravity', gravity)) if on)
    if not terms:
        raise ValueError('cloth_energy: select at least one term')
    _float32('cloth_energy', x)
    total, energy = _Energy.apply(x, garment.cloth, terms, float(g))
    return (total, energy) if per_term else total


def stretch_energy(v: torch.Tensor, garment: Garment):
    """v (B,V,3) -> the StVK membrane energy, summed over the faces and divided by B"""
    return cloth_energy(v, garment, stretch=True, bending=False)


def bending_energy(v: torch.Tensor, garment: Garment):
    """v (B,V,3) -> the dihedral-angle bending energy (signed form), summed over the manifold edges and divided by B"""
    return cloth_energy(v, garment, stretch=False, bending=True)


class _Rows(torch.autograd.Function):
    """sum over rows of ra_cloth_inertia / rows, with the three gradients"""

    @staticmethod
    def forward(ctx, x_next, x_curr, v_curr, mass, delta_t, accel, engine):
        need = tuple(ctx.needs_input_grad[:3])
        value, *grads = engine.cloth_inertia(mass, x_next, x_curr, v_curr, delta_t, accel, grads=need)
        ctx.grads, ctx.rows = grads, x_next.shape[0]
        return (value.sum() / x_next.shape[0]).to(torch.float32)

    @staticmethod
    def backward(ctx, d):
        s = d / ctx.rows
        return (*[None if g is None else g * s.to(g.dtype) for g in ctx.grads], None, None, None, None)


def gravity_energy(x: torch.Tensor, mass: torch.Tensor, g=9.81):
    """x (S,V,3), mass (V,) -> sum(g mass y) / S.  The reference takes the mass as a tensor, not a Garment: a gather-free product,
    plain torch (cloth_energy(gravity=True) is the fused form)"""
    return torch.sum(g * mass * x[:, :, 1]) / x.shape[0]


def inertia_term(x_next: torch.Tensor, x_curr: torch.Tensor, v_curr: torch.Tensor, mass: torch.Tensor, delta_t, engine=None):
    _float32('inertia_term', x_next, x_curr, v_curr)
    return _Rows.apply(x_next, x_curr, v_curr, mass, float(delta_t), None, _engine(engine))


def dynamic_term(x_next: torch.Tensor, x_curr: torch.Tensor, v_curr: torch.Tensor, mass: torch.Tensor, delta_t,
                 gravitational_acceleration=[0, -9.81, 0], engine=None):
    _float32('dynamic_term', x_next, x_curr, v_curr)
    return _Rows.apply(x_next, x_curr, v_curr, mass, float(delta_t), tuple(float(a) for a in gravitational_acceleration), _engine(engine))


def inertia_term_sequence(x: torch.Tensor, mass: torch.Tensor, delta_t: float, method: Callable = inertia_term, compliance: float = 1.0):
    """x (B,T,V,3) -> compliance x method over the B (T - 1) frame pairs of every sequence: frame t + 1 against frame t, with the
    finite-difference velocity that ARRIVED at frame t (none arrives at the first frame: 0).  Any B: the reference's own view() only
    accepts B = 1."""
    V = x.shape[-2]
    velocity = torch.diff(x, dim=1) / delta_t                                        # B, T - 1: the one that leaves frame t
    arriving = torch.nn.functional.pad(velocity[:, :-1], (0, 0, 0, 0, 1, 0))         # shifted by one frame, zeros in front
    later, earlier, arriving = (t.reshape(-1, V, 3) for t in (x[:, 1:], x[:, :-1], arriving))
    return compliance * method(later, earlier, arriving, mass, delta_t)


def xpbd_constraints(*args, **kwargs):
    raise NotImplementedError('xpbd_constraints: ' + XPBD_REASON)


def stretch_energy_constraints(*args, **kwargs):
    raise NotImplementedError('stretch_energy_constraints: ' + XPBD_REASON)


def bending_energy_constraints(*args, **kwargs):
    raise NotImplementedError('bending_energy_constraints: ' + XPBD_REASON)

"""The lifecycle that Mesh, Topology and Cloth share (relightableavatar_amd/handles.py; ra_mesh_destroy, ra_topo_destroy and
ra_cloth_destroy of the C ABI), the same for all three: a handle answers, refuses once closed, refuses once its engine's context is gone,
and is destroyed only through the context that owns it.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import pytest
import torch

from relightableavatar_amd import _lib
from relightableavatar_amd.config import make_cfg

pytestmark = pytest.mark.gpu
# an octahedron: 6 vertices, 8 faces, closed and outward-facing
VERTS = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float32)
FACES = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=torch.int32)


@pytest.fixture(scope='module')
def eng():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from relightableavatar_amd.engine import Engine
    return Engine(make_cfg('relight'), device='cuda:0')          # any context will do: no weights are read


def make(kind, e):
    """-> (the handle, a query of it, the handles to close after it)"""
    if kind == 'mesh':
        h = e.mesh(VERTS, FACES)
        return h, lambda: h.closest(VERTS * 2).d2.shape == (6,), ()
    topo = e.topology(FACES, 6)
    if kind == 'topology':
        return topo, lambda: topo.smooth(VERTS, iter=2).shape == (6, 3), ()
    h = e.cloth(topo, VERTS, VERTS[:, :2], FACES)       # default material; a face spans a triangle of area 1/2 in the first two coordinates
    return h, lambda: h.energy(VERTS[None])[0].shape == (1, 3), (topo,)


@pytest.mark.parametrize('kind', ('mesh', 'topology', 'cloth'))
def test_handle_lifecycle(eng, kind):
    from relightableavatar_amd.engine import Engine
    noun, destroy = kind.capitalize(), getattr(eng.lib, {'mesh': 'ra_mesh_destroy', 'topology': 'ra_topo_destroy', 'cloth': 'ra_cloth_destroy'}[kind])
    h, query, rest = make(kind, eng)
    assert query()
    # a handle belongs to its context: another one's destroy entry refuses it
    other = Engine(make_cfg('relight'), device='cuda:0')
    assert destroy(other.ctx, h._handle) != 0
    assert f'not a {kind} of this ctx' in eng.lib.ra_last_error().decode()
    assert query()
    # closed: the same query refuses; closing again is harmless
    h.close()
    with pytest.raises(_lib.RaError, match=f'{noun}: closed'):
        query()
    h.close()
    for r in rest:
        r.close()
    # the context frees what is left; the handle then only refuses, and close() only forgets
    orphan, orphan_query, orphan_rest = make(kind, other)
    assert orphan_query()
    eng.lib.ra_ctx_destroy(other.ctx)
    other.ctx = C.c_void_p()
    with pytest.raises(_lib.RaError, match=f'{noun}: the engine that built this {kind} is gone'):
        orphan_query()
    orphan.close()
    for r in orphan_rest:
        r.close()

"""The 256-entry tables of marching cubes (csrc/ra_mcubes.hip), derived by rule instead of copied.

Corner and edge numbering are the classic ones: corners 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1), edges
0..3 round the z = 0 face, 4..7 round the z = 1 face, 8..11 the four along z; bit k of a cell's case is set when corner k is BELOW
the iso value (v < iso).

Per case:
  - a cube edge carries a vertex when its two corners differ;
  - on each of the six cube faces the crossed edges are joined by segments: two crossed edges by one segment, four (the ambiguous
    face: the corners alternate) by two segments that each cut off one BELOW corner.  The pairing depends on the four corner signs of
    the face alone, so the two cells that share a face draw the same segments: the surface has no cracks, on any volume;
  - a segment is directed so that, seen from outside the cube, the below corners are on its left.  The two faces at a cube edge then
    give its vertex one segment in and one out, and the segments close into directed loops whose right-hand normal points towards the
    below corners: towards SMALLER volume values;
  - a loop starts at its lowest edge and the loops are ordered by that edge; a loop of more than three vertices is cut into triangles
    so that as few diagonals as possible join two vertices of one cube face (such a diagonal can coincide with the neighbour cell's
    and give a mesh edge four faces), the first such triangulation in lexicographic order of the split points.

This is the classic algorithm with the classic numbering; the triangulation of a case is NOT promised to be the one of Lorensen &
Cline's or Bourke's printed table, and a case may take more than five triangles (MAX_TRI).

`python -m relightableavatar_amd.mcubes_tables` prints csrc/ra_mcubes_tables.hpp; a test keeps the two equal."""
import functools

import numpy as np

CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGE_CORNERS = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
# the grid point that owns an edge (offset from the cell's minimum corner) and the axis the edge runs along
EDGE_OWNER = tuple(tuple(min(CORNERS[a][k], CORNERS[b][k]) for k in range(3)) for a, b in EDGE_CORNERS)
EDGE_AXIS = tuple(next(k for k in range(3) if CORNERS[a][k] != CORNERS[b][k]) for a, b in EDGE_CORNERS)


def _faces():
    """the six cube faces: (outward normal, corners in cyclic order, the edge between corner i and corner i + 1)"""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            # cyclic order: walk the square
            u, v = [k for k in range(3) if k != axis]
            order = sorted(cs, key=lambda c: {(0, 0): 0, (1, 0): 1, (1, 1): 2, (0, 1): 3}[(CORNERS[c][u], CORNERS[c][v])])
            edges = []
            for i in range(4):
                pair = {order[i], order[(i + 1) % 4]}
                edges.append(next(e for e, ab in enumerate(EDGE_CORNERS) if set(ab) == pair))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((tuple(n), tuple(order), tuple(edges)))
    return out


FACES = _faces()
_SAME_FACE = {(a, b) for _, _, es in FACES for a in es for b in es}


def _mid(e):
    a, b = EDGE_CORNERS[e]
    return np.array([(CORNERS[a][k] + CORNERS[b][k]) / 2 for k in range(3)])


def _segments(case):
    """directed segments (from edge, to edge) of a case"""
    below = [(case >> c) & 1 for c in range(8)]
    segs = []
    for n, cs, es in FACES:
        crossed = [i for i in range(4) if below[cs[i]] != below[cs[(i + 1) % 4]]]
        if len(crossed) == 2:
            pairs = [(es[crossed[0]], es[crossed[1]], next(c for c in cs if below[c]))]
        elif len(crossed) == 4:
            # corner i sits between edge i - 1 and edge i: cut off every below corner
            pairs = [(es[(i - 1) % 4], es[i], cs[i]) for i in range(4) if below[cs[i]]]
        else:
            continue
        for a, b, c in pairs:
            pa, pb, pc = _mid(a), _mid(b), np.array(CORNERS[c], dtype=float)
            left = float(np.dot(n, np.cross(pb - pa, pc - pa)))
            assert left != 0.0
            segs.append((a, b) if left > 0 else (b, a))
    return segs


def _loops(case):
    nxt = {}
    for a, b in _segments(case):
        assert a not in nxt
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop, k = [], e
        while k not in seen:
            seen.add(k)
            loop.append(k)
            k = nxt[k]
        assert k == e
        loops.append(loop)
    return loops


def _triangulate(loop):
    """(bad diagonals, triangles) of a directed loop, each triangle in the loop's direction"""
    loop = tuple(loop)

    @functools.lru_cache(maxsize=None)
    def best(i, j):     # the polygon loop[i..j], closed by the chord (i, j)
        if j - i < 2:
            return 0, ()
        res = None
        for k in range(i + 1, j):
            bad = 0
            for a, b in ((i, k), (k, j)):
                if b - a > 1 and (loop[a], loop[b]) in _SAME_FACE:
                    bad += 1
            l, r = best(i, k), best(k, j)
            cand = (bad + l[0] + r[0], ((loop[i], loop[k], loop[j]),) + l[1] + r[1])
            if res is None or cand[0] < res[0]:
                res = cand
        return res

    return best(0, len(loop) - 1)


@functools.lru_cache(maxsize=None)
def build_tables():
    """edge_table (256,) int32: bit e set when edge e is crossed; n_tri (256,) int32; tri_table (256, 3 * MAX_TRI) int32, -1 padded;
    bad (256,) int32: diagonals of the case that lie in a cube face"""
    edge_table = np.zeros(256, np.int32)
    tris, bad = [], np.zeros(256, np.int32)
    for case in range(256):
        for e, (a, b) in enumerate(EDGE_CORNERS):
            if ((case >> a) & 1) != ((case >> b) & 1):
                edge_table[case] |= 1 << e
        t = []
        for loop in _loops(case):
            nb, tt = _triangulate(loop)
            bad[case] += nb
            t += [e for tri in tt for e in tri]
        assert set(t) == {e for e in range(12) if edge_table[case] >> e & 1}
        tris.append(t)
    max_tri = max(len(t) for t in tris) // 3
    tri_table = np.full((256, 3 * max_tri), -1, np.int32)
    for case, t in enumerate(tris):
        tri_table[case, :len(t)] = t
    n_tri = np.array([len(t) // 3 for t in tris], np.int32)
    return edge_table, n_tri, tri_table, bad


MAX_TRI = build_tables()[2].shape[1] // 3


def header_text():
    edge_table, n_tri, tri_table, _ = build_tables()
    rows = lambda a, per: ',\n'.join('    ' + ', '.join(str(int(v)) for v in a[i:i + per]) for i in range(0, len(a), per))
    return ('// Generated by `python -m relightableavatar_amd.mcubes_tables`: do not edit (tests/test_oracle_mesh_extract.py keeps it equal).\n'
            '// The marching-cubes tables: how they are derived is written in relightableavatar_amd/mcubes_tables.py.\n'
            '#pragma once\n'
            f'constexpr int MC_MAX_TRI = {MAX_TRI};\n'
            '// triangles of a case\n'
            f'__device__ const unsigned char MC_NTRI[256] = {{\n{rows(n_tri, 32)}}};\n'
            '// per case 3 * MC_MAX_TRI cube edges, three per triangle (unused slots: 255)\n'
            f'__device__ const unsigned char MC_TRI[256 * {3 * MAX_TRI}] = {{\n{rows(np.where(tri_table < 0, 255, tri_table).reshape(-1), 3 * MAX_TRI)}}};\n'
            '// per cube edge: the owning grid point as (dx | dy << 1 | dz << 2) from the cell\'s minimum corner, and the axis (0 x, 1 y, 2 z)\n'
            f'__device__ const unsigned char MC_EDGE_OWNER[12] = {{{", ".join(str(o[0] | o[1] << 1 | o[2] << 2) for o in EDGE_OWNER)}}};\n'
            f'__device__ const unsigned char MC_EDGE_AXIS[12] = {{{", ".join(str(a) for a in EDGE_AXIS)}}};\n')


if __name__ == '__main__':
    print(header_text(), end='')

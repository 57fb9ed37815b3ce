"""The 256-case marching-cubes triangle table, generated (not typed), and its C++ form.

    python -m loner_amd.mc_table          # rewrites loner_amd/csrc/mc_table.hpp

Conventions (shared by ``meshing.marching_cubes_ref`` and csrc/mesh.hip):
  corner c    = dx + 2 dy + 4 dz of the cell's lower corner; bit c of the case is set when that corner is INSIDE
                (value > level)
  edge e      = 4 axis + j: the grid edge along ``axis`` whose lower end is the corner at offset EDGE_OFFSET[e]
                (the two other axes, in increasing order, take the bits j & 1 and j >> 1)
  TRI_TABLE   (256, 3 MAX_TRIS) int8: edge triples, -1 padded; TRI_COUNT (256,) the triangles per case

Construction: on each of the cell's six faces the crossed edges are joined by segments.  A face with two crossed edges
has one segment; a face with four (inside corners on one diagonal: the ambiguous face) gets two segments that each cut
off ONE INSIDE corner.  The rule reads only the face's own four corners, so the two cells that share a face draw the
same segments on it and the surface has no holes (the classic table resolves such a face by case complement, which
two neighbours can do differently).  Every crossed edge lies on two faces and ends one segment on each, so the
segments close into loops; each loop is cut into triangles without a diagonal between two edges of one face (such a
diagonal lies in the face, where the neighbour may draw it too).  Segments are directed with the inside corner on one
fixed side as seen from outside the cell, which winds every triangle so that its normal points from inside to outside.
"""
import os

import numpy as np

CORNER = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
EDGE_AXIS = np.array([e >> 2 for e in range(12)], np.int64)


def _edge_offset(e):
    axis, j = e >> 2, e & 3
    u, v = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[u], off[v] = j & 1, j >> 1
    return off


EDGE_OFFSET = np.array([_edge_offset(e) for e in range(12)], np.int64)


def _corner_id(p):
    return int(p[0] + 2 * p[1] + 4 * p[2])


def _edge_between(p, q):
    """The edge whose ends are the adjacent corners p and q."""
    lo = np.minimum(p, q)
    axis = int(np.flatnonzero(p != q)[0])
    for e in range(12):
        if EDGE_AXIS[e] == axis and (EDGE_OFFSET[e] == lo).all():
            return e
    raise AssertionError


def _case_loops(case):
    inside = [(case >> c) & 1 for c in range(8)]
    mid = EDGE_OFFSET.astype(np.float64)
    mid[np.arange(12), EDGE_AXIS] += 0.5
    nxt = {}
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            normal = np.zeros(3)
            normal[axis] = 1.0 if side else -1.0
            ring = []  # the face's corners in cyclic order
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = np.zeros(3, np.int64)
                p[axis], p[u], p[v] = side, du, dv
                ring.append(p)
            ins = [inside[_corner_id(p)] for p in ring]
            edges = [_edge_between(ring[k], ring[(k + 1) % 4]) for k in range(4)]  # edge k joins corners k, k + 1
            crossed = [k for k in range(4) if ins[k] != ins[(k + 1) % 4]]
            segs = []  # (edge, edge, an inside corner on the segment's inside)
            if len(crossed) == 2:
                segs.append((edges[crossed[0]], edges[crossed[1]], ring[ins.index(1)]))
            elif len(crossed) == 4:
                for k in range(4):
                    if ins[k]:  # cut off inside corner k: its two edges are k - 1 and k
                        segs.append((edges[(k - 1) % 4], edges[k], ring[k]))
            for a, b, c in segs:
                if np.dot(normal, np.cross(mid[b] - mid[a], c - mid[a])) < 0:
                    a, b = b, a
                assert a not in nxt, "an edge starts two segments"
                nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), "the segments do not close"
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        loops.append(loop)
    return loops


def _share_face(e, f):
    """Do the cell edges e and f lie on a common face of the cell?"""
    pe = [EDGE_OFFSET[e], EDGE_OFFSET[e] + np.eye(3, dtype=np.int64)[EDGE_AXIS[e]]]
    pf = [EDGE_OFFSET[f], EDGE_OFFSET[f] + np.eye(3, dtype=np.int64)[EDGE_AXIS[f]]]
    return any(all(p[a] == s for p in pe + pf) for a in range(3) for s in (0, 1))


def _triangulate(loop):
    """The first triangulation (in a fixed search order) of the polygon ``loop`` none of whose diagonals joins two
    edges of one cell face: such a diagonal lies in the face, where the neighbouring cell may draw it too, and the
    mesh edge would then carry four triangles."""
    n = len(loop)

    def ok(i, j):
        return (j - i) in (1, n - 1) or not _share_face(loop[i], loop[j])

    def rec(i, j):  # the polygon loop[i..j], closed by the (allowed) chord i-j
        if j - i < 2:
            return []
        for k in range(i + 1, j):
            if ok(i, k) and ok(k, j):
                a, b = rec(i, k), rec(k, j)
                if a is not None and b is not None:
                    return [(i, k, j)] + a + b
        return None

    t = rec(0, n - 1)
    assert t is not None, f"no triangulation of {loop} without a diagonal in a face"
    # the loop runs clockwise seen from outside (inside on the left of a segment seen from outside the CELL)
    return [(loop[i], loop[j], loop[k]) for i, k, j in t]


def generate():
    """-> (TRI_TABLE (256, 3 MAX_TRIS) int8, TRI_COUNT (256,) uint8)."""
    tris = []
    for case in range(256):
        t = []
        for loop in _case_loops(case):
            t += _triangulate(loop)
        tris.append(t)
    # the winding, checked where it is plain: one inside corner, the normal points away from it
    mid = EDGE_OFFSET.astype(np.float64)
    mid[np.arange(12), EDGE_AXIS] += 0.5
    for c in range(8):
        (a, b, d), = tris[1 << c]
        n = np.cross(mid[b] - mid[a], mid[d] - mid[a])
        assert np.dot(n, (mid[a] + mid[b] + mid[d]) / 3 - CORNER[c]) > 0, "triangles wound inwards"
    max_tris = max(len(t) for t in tris)
    table = np.full((256, 3 * max_tris), -1, np.int8)
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri]
        table[case, :len(flat)] = flat
    return table, np.array([len(t) for t in tris], np.uint8)


TRI_TABLE, TRI_COUNT = generate()
MAX_TRIS = TRI_TABLE.shape[1] // 3

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.hpp")


def header_text():
    rows = ",\n".join("    {" + ", ".join(f"{int(v):2d}" for v in row) + "}" for row in TRI_TABLE)
    counts = ",\n".join("    " + ", ".join(str(int(v)) for v in TRI_COUNT[i:i + 32]) for i in range(0, 256, 32))
    return ("// Generated by `python -m loner_amd.mc_table`; do not edit (tests/test_meshing_ref.py compares it\n"
            "// with the generator).  Conventions: loner_amd/mc_table.py.\n"
            "#pragma once\n#include <cstdint>\n\nnamespace lnr {\n\n"
            f"constexpr int kMcMaxTris = {MAX_TRIS};\n"
            f"static __device__ const int8_t kMcTriTable[256][{3 * MAX_TRIS}] = {{\n{rows}}};\n"
            f"static __device__ const uint8_t kMcTriCount[256] = {{\n{counts}}};\n\n"
            "}  // namespace lnr\n")


if __name__ == "__main__":
    with open(HEADER_PATH, "w") as f:
        f.write(header_text())
    print(HEADER_PATH, "max triangles per cell:", MAX_TRIS)

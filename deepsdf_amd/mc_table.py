"""Generator of the marching-cubes case table (csrc/mc_table.hpp).  No dependencies beyond the standard library.

    python -m deepsdf_amd.mc_table            # rewrites deepsdf_amd/csrc/mc_table.hpp

Conventions (shared with csrc/mcubes.hpp and the tests):
  corner c of a cell at grid point p = (i, j, k) is p + (c & 1, (c >> 1) & 1, (c >> 2) & 1); axis 0 (x) is the slowest grid axis.
  case = sum of (1 << c) over the corners that are INSIDE (value < level, strictly).
  edge e = 4 * axis + k runs from corner EDGES[e][0] along EDGES[e][1]; k enumerates the corners whose `axis` bit is clear.

The table is built, not typed:
  1. on each of the 6 cube faces, the crossing edges are paired into segments from that face's 4 corner signs alone; on an
     ambiguous face (the two inside corners diagonal) every inside corner is cut off by its own segment (inside separated);
  2. each segment is oriented so that, seen from outside the cell, the inside corners it cuts off lie on its RIGHT.  The
     neighbour across the face sees the face from the other side, so it traverses the same segment the other way round;
  3. the segments chain into closed loops (every crossing edge ends one segment and starts one), and each loop is
     fan-triangulated.  With orientation 2, the right-hand-rule normal of every triangle points from the inside corners
     towards the outside ones, i.e. towards increasing SDF (outward).
"""
import os

EDGES = [(c, a) for a in range(3) for c in range(8) if not (c >> a) & 1]   # 12 (corner, axis), edge id = index


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_id(c, a):
    return EDGES.index((c, a))


def edge_mid(e):
    c, a = EDGES[e]
    p = list(map(float, corner_pos(c)))
    p[a] += 0.5
    return p


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return sum(a * b for a, b in zip(u, v))


def _sub(u, v):
    return tuple(a - b for a, b in zip(u, v))


def face_corners(f, s):
    """The 4 corners of cube face (axis f, side s) in cyclic order."""
    u, v = (f + 1) % 3, (f + 2) % 3
    return [(s << f) | (qu << u) | (qv << v) for qu, qv in ((0, 0), (1, 0), (1, 1), (0, 1))]


def _edge_between(c0, c1):
    a = (c0 ^ c1).bit_length() - 1
    return edge_id(min(c0, c1), a)


def face_segments(case, f, s):
    """Directed segments (edge_from, edge_to) of `case` on face (f, s), from that face's corner signs only."""
    q = face_corners(f, s)
    inside = [(case >> c) & 1 for c in q]
    cross = [i for i in range(4) if inside[i] != inside[(i + 1) % 4]]      # face edge i joins q[i] and q[i+1]
    if not cross:
        return []
    if len(cross) == 2:
        groups = [((cross[0], cross[1]), [q[i] for i in range(4) if inside[i]])]
    else:      # ambiguous: the inside corners q[i] are separated, each cut off by the segment of its two face edges
        groups = [(((i - 1) % 4, i), [q[i]]) for i in range(4) if inside[i]]
    n = [0.0, 0.0, 0.0]
    n[f] = 1.0 if s else -1.0
    segs = []
    for (i0, i1), cut in groups:
        e0 = _edge_between(q[i0], q[(i0 + 1) % 4])
        e1 = _edge_between(q[i1], q[(i1 + 1) % 4])
        p0, p1 = edge_mid(e0), edge_mid(e1)
        mid = [(a + b) / 2 for a, b in zip(p0, p1)]
        cen = [sum(corner_pos(c)[k] for c in cut) / len(cut) for k in range(3)]
        left = _cross(n, _sub(p1, p0))
        if _dot(left, _sub(cen, mid)) > 0:     # inside on the left: turn round, the inside goes on the right
            e0, e1 = e1, e0
        segs.append((e0, e1))
    return segs


def case_loops(case):
    nxt = {}
    for f in range(3):
        for s in range(2):
            for e0, e1 in face_segments(case, f, s):
                assert e0 not in nxt, (case, e0)
                nxt[e0] = e1
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


TABLE = [case_triangles(c) for c in range(256)]
MAX_TRIS = max(len(t) for t in TABLE)
WIDTH = 3 * MAX_TRIS + 1          # a row: edge ids, -1 terminated


def _check_orientation():
    """Case 1 (corner 0 inside): the triangle's normal must point away from corner 0 (towards increasing SDF)."""
    (a, b, c), = TABLE[1]
    pa, pb, pc = edge_mid(a), edge_mid(b), edge_mid(c)
    nrm = _cross(_sub(pb, pa), _sub(pc, pa))
    assert _dot(nrm, (1, 1, 1)) > 0


_check_orientation()


def table_rows():
    """256 rows of WIDTH int8: edge ids of the case's triangles, then -1 up to WIDTH."""
    return [[e for t in tris for e in t] + [-1] * (WIDTH - 3 * len(tris)) for tris in TABLE]


def header_text():
    rows = table_rows()
    out = ["// mc_table.hpp -- GENERATED by deepsdf_amd/mc_table.py (python -m deepsdf_amd.mc_table); do not edit.",
           "// Marching-cubes case table: conventions in deepsdf_amd/mc_table.py.",
           "#pragma once", "#include <stdint.h>", "",
           "namespace dsdf {", "",
           f"constexpr int MC_MAX_TRIS = {MAX_TRIS};",
           f"constexpr int MC_TABLE_W = {WIDTH};   // edge ids of a case's triangles, -1 terminated", "",
           "// edge e: (lower corner, axis)",
           "#define DSDF_MC_EDGES_INIT {" + ", ".join(f"{{{c}, {a}}}" for c, a in EDGES) + "}", "",
           "#define DSDF_MC_NTRI_INIT {" + ", ".join(str(len(t)) for t in TABLE) + "}", "",
           "#define DSDF_MC_TRI_INIT { \\"]
    for c, r in enumerate(rows):
        out.append("  {" + ", ".join(str(e) for e in r) + "}" + ("," if c < 255 else "") + " \\")
    out += ["}", "", "}  // namespace dsdf", ""]
    return "\n".join(out)


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.hpp")


def write_header(path=HEADER):
    with open(path, "w") as f:
        f.write(header_text())
    return path


if __name__ == "__main__":
    print(write_header(), "max triangles per case:", MAX_TRIS)

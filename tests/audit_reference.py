"""The mesh audit restated in numpy (not a test).

An independent statement of what ``pr_mesh_audit`` (include/playrender.h) returns, written from the header's words and without a hash
table: vertex classes from ``np.unique`` over the components (-0 folded to +0), edges from ``np.unique`` over the pairs of
representatives, shells by label propagation over the edges, the measures as plain float64 sums.  ``audit`` also returns the sums of
the absolute terms, from which the tests derive the header's bound ``T_g 2^-52 sum|term|`` for the device's fixed summation tree.
Nothing here imports the package.
"""
import numpy as np

from tests.raycast_reference import clamped_offsets, group_slices

F = np.float32
FIELDS = ("candidates", "dropped", "vertices", "edges", "unbalanced_edges", "boundary_edges", "non_manifold_edges",
          "euler_characteristic", "shells", "largest_shell")


def representatives(vertices):
    """``(V)`` int64: per vertex the lowest index with the same three values (== on fp32, so -0 is +0), -1 where a component is not
    finite."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    rep = np.full(len(v), -1, dtype=np.int64)
    finite = np.isfinite(v).all(axis=1)
    if finite.any():
        index = np.nonzero(finite)[0]
        values = v[index] + F(0)                                    # -0 + 0 = +0: one bit pattern per value
        _, first, inverse = np.unique(values, axis=0, return_index=True, return_inverse=True)
        rep[index] = index[first][inverse.reshape(-1)]              # (np.unique returns the first occurrence: the lowest index)
    return rep


def candidate_mask(vertices, triangles, rep):
    """``(T)`` bool by the header: three indices in [0, V_g), nine finite coordinates, neither a == b nor a == c as values."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0 or len(vertices) == 0:
        return np.zeros(len(t), dtype=bool)
    valid = np.all((t >= 0) & (t < len(vertices)), axis=1)
    r = rep[np.where(valid[:, None], t, 0)]
    return valid & (r >= 0).all(axis=1) & (r[:, 0] != r[:, 1]) & (r[:, 0] != r[:, 2])


def _shells(T, sides_triangle, sides_edge, candidate):
    """Labels ``(T)``: per candidate the lowest triangle index of its shell, -1 otherwise.  Label propagation: every triangle takes the
    minimum over its edges, every edge the minimum over its triangles, until nothing changes."""
    label = np.where(candidate, np.arange(T), -1).astype(np.int64)
    if len(sides_edge) == 0:
        return label
    edges = int(sides_edge.max()) + 1
    while True:
        lowest = np.full(edges, T, dtype=np.int64)
        np.minimum.at(lowest, sides_edge, label[sides_triangle])
        new = label.copy()
        np.minimum.at(new, sides_triangle, lowest[sides_edge])
        if np.array_equal(new, label):
            return label
        label = new


def audit_group(vertices, triangles):
    """One group: ``(counts (12) int64, measures (8), absolute (5), labels (T_g) int64)``."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    T = len(t)
    counts, measures, absolute = np.zeros(12, dtype=np.int64), np.zeros(8), np.zeros(5)
    rep = representatives(v)
    cand = candidate_mask(v, t, rep)
    counts[0], counts[1] = int(cand.sum()), int(T - cand.sum())
    labels = np.full(T, -1, dtype=np.int64)
    if not cand.any():
        return counts, measures, absolute, labels
    rows = np.nonzero(cand)[0]
    r = rep[t[rows]]
    # the three sides a -> b, b -> c, c -> a; one with equal ends is no edge
    start, end = np.concatenate([r[:, 0], r[:, 1], r[:, 2]]), np.concatenate([r[:, 1], r[:, 2], r[:, 0]])
    owner = np.concatenate([rows, rows, rows])
    proper = start != end
    start, end, owner = start[proper], end[proper], owner[proper]
    low, high = np.minimum(start, end), np.maximum(start, end)
    pairs, edge = np.unique(np.stack([low, high], axis=1), axis=0, return_inverse=True)
    edge = edge.reshape(-1)
    E = len(pairs)
    forward = np.bincount(edge, weights=(start == low), minlength=E).astype(np.int64)
    backward = np.bincount(edge, weights=(start != low), minlength=E).astype(np.int64)
    counts[2] = len(np.unique(np.concatenate([start, end])))
    counts[3] = E
    counts[4] = int((forward != backward).sum())
    counts[5] = int((forward + backward == 1).sum())
    counts[6] = int((forward + backward > 2).sum())
    counts[7] = counts[2] - counts[3] + counts[0]
    labels = _shells(T, owner, edge, cand)
    roots, sizes = np.unique(labels[cand], return_counts=True)
    counts[8], counts[9] = len(roots), int(sizes.max())
    # the measures: the header's expressions in float64, summed plainly
    a, b, c = (v[t[rows, k]].astype(np.float64) for k in range(3))
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    m0 = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    m1 = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    m2 = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    volume = ((a[:, 0] * m0 + a[:, 1] * m1) + a[:, 2] * m2) / 6.0
    weighted = area[:, None] * (((a + b) + c) / 3.0)
    measures[0], measures[1] = area.sum(), volume.sum()
    measures[2:5] = weighted.sum(axis=0) / measures[0] if measures[0] > 0 else 0.0
    absolute[0], absolute[1] = np.abs(area).sum(), np.abs(volume).sum()
    absolute[2:5] = np.abs(weighted).sum(axis=0)
    return counts, measures, absolute, labels


def audit(mesh):
    """``mesh``: the packed dict of tests/surface_reference.py (optionally with the totals ``V`` / ``T``).  Returns a dict: ``counts
    (G, 12)`` int32, ``measures (G, 8)`` float64, ``absolute (G, 5)`` float64 - the sums of |term| of area, volume and the three centroid
    sums -, ``labels (T)`` int32 (-1 also for the rows that no clamped group owns)."""
    t = np.asarray(mesh["triangles"]).reshape(-1, 3)
    T = int(mesh.get("T", len(t)))
    to = clamped_offsets(mesh["triangle_offsets"], T)
    parts = [audit_group(vertices, triangles) for vertices, triangles in group_slices(mesh)]
    labels = np.full(T, -1, dtype=np.int32)
    for g, p in enumerate(parts):
        labels[to[g]:to[g + 1]] = p[3]
    return {"counts": np.stack([p[0] for p in parts]).astype(np.int32), "measures": np.stack([p[1] for p in parts]),
            "absolute": np.stack([p[2] for p in parts]), "labels": labels}


def bounds(reference):
    """``(G, 8)``: the header's bound on |device - reference| per measure: ``T_g 2^-52 sum|term|`` for area and volume, the same for
    the centroid sums, carried through the division by the area (the sum's bound over the area, plus the centroid's magnitude bound
    sum|term| / area times the area's relative bound, plus one rounding of either side's division) - fp64 summation of T_g terms, no
    measured tolerance."""
    counts, absolute, measures = reference["counts"].astype(np.float64), reference["absolute"], reference["measures"]
    eps = (counts[:, 0] + counts[:, 1]) * 2.0 ** -52                          # T_g = candidates + dropped
    out = np.zeros_like(measures)
    out[:, 0:2] = eps[:, None] * absolute[:, 0:2]
    area = np.where(measures[:, 0] > 0, measures[:, 0], 1.0)
    magnitude = absolute[:, 2:5] / area[:, None]                              # >= |centroid component|
    out[:, 2:5] = (eps[:, None] * absolute[:, 2:5] + magnitude * out[:, 0:1]) / area[:, None] + 2.0 ** -52 * magnitude      # (+ the two divisions)
    return out


def report(counts, measures):
    """The dict ``surface.MeshAudit.report`` returns, from one row of counts and measures."""
    out = {name: int(counts[i]) for i, name in enumerate(FIELDS)}
    out["area"], out["signed_volume"], out["centroid"] = float(measures[0]), float(measures[1]), [float(x) for x in measures[2:5]]
    out["balanced"] = out["unbalanced_edges"] == 0
    out["closed_manifold"] = out["balanced"] and out["boundary_edges"] == 0 and out["non_manifold_edges"] == 0
    return out


# ------------------------------------------------------------------------------------------------ the meshes the tests share
def two_spheres(radii=(0.31, 0.31), n=17):
    """One group that holds two disjoint spheres (centres -0.47 and +0.47 on x; no lattice value equals the level): the packed
    single-group dict.  The sphere at -0.47 comes first in the triangle order."""
    from tests import surface_reference as sr
    x = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    field = np.maximum(radii[0] ** 2 - ((X + 0.47) ** 2 + Y * Y + Z * Z), radii[1] ** 2 - ((X - 0.47) ** 2 + Y * Y + Z * Z)).astype(F)
    return sr.extract_surface(field[None], [x.astype(F)] * 3, 0.0)


def duplicated_tetrahedron():
    """A closed tetrahedron in which every triangle has three vertices of its own (12 vertices, four values): every directed edge has
    its reverse by VALUE and none by index."""
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F)
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    return {"vertices": corners[faces.reshape(-1)].copy(), "triangles": np.arange(12, dtype=np.int32).reshape(4, 3),
            "vertex_offsets": np.array([0, 12], dtype=np.int32), "triangle_offsets": np.array([0, 4], dtype=np.int32)}


def hand_made():
    """A small hostile group: NaN / inf vertices, indices -1 / V_g / 2^31 - 1, a == b, a == c, b == c, -0 against +0, a triangle listed
    twice and once reversed - and its expected counts, derived by hand below."""
    nan, inf = np.nan, np.inf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],             # 0..3: a tetrahedron
                  [-0.0, 0.0, -0.0],                                      # 4: vertex 0 again, by value
                  [1, 0, 0],                                              # 5: vertex 1 again
                  [nan, 0, 0], [0, inf, 0], [0, 0, -inf],                 # 6..8: not finite
                  [2, 2, 2]], dtype=F)                                    # 9: referenced only by dropped triangles
    t = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [4, 3, 2],             # 0..3: the closed tetrahedron (one corner through its twin)
                  [0, 1, 3], [0, 1, 3], [3, 1, 0],                        # 4..6: triangle 1 twice more, and once reversed
                  [0, 4, 1],                                              # 7: a == b by value: dropped
                  [0, 1, 4],                                              # 8: a == c by value: dropped
                  [2, 5, 1],                                              # 9: b == c by value: a candidate, sides 2 -> 1 and 1 -> 2
                  [-1, 1, 2], [0, 10, 2], [0, 1, 2 ** 31 - 1],            # 10..12: an index out of range: dropped
                  [6, 1, 2], [0, 7, 2], [0, 1, 8],                        # 13..15: a vertex that is not finite: dropped
                  [9, 9, 9]], dtype=np.int32)                             # 16: a == b: dropped
    mesh = {"vertices": v, "triangles": t, "vertex_offsets": np.array([0, len(v)], dtype=np.int32),
            "triangle_offsets": np.array([0, len(t)], dtype=np.int32)}
    # candidates 0..6 and 9; classes {0, 4}, {1, 5}, 2, 3 are referenced: Vr = 4; edges: the tetrahedron's six.  Edge {0, 1}: sides
    # 0 -> 1 from triangles 1, 4, 5 and 1 -> 0 from 0 and 6: f = 3, b = 2, unbalanced and non-manifold.  Edge {1, 3}: 1 -> 3 from 1, 4, 5
    # and 3 -> 1 from 2 and 6: the same.  Edge {0, 3}: 3 -> 0 from 1, 4, 5 and 0 -> 3 from 3 and 6: the same.  Edge {1, 2}: 2 -> 1 from 0
    # and 9, 1 -> 2 from 2 and 9: f = b = 2, balanced, non-manifold.  Edges {0, 2}, {2, 3}: once each way.  One shell of 8.
    expected = {"candidates": 8, "dropped": 9, "vertices": 4, "edges": 6, "unbalanced_edges": 3, "boundary_edges": 0,
                "non_manifold_edges": 4, "euler_characteristic": 4 - 6 + 8, "shells": 1, "largest_shell": 8}
    return mesh, expected

"""Vertex clustering on a uniform grid, restated in numpy (not a test).

An independent statement of what ``pr_simplify_mesh`` (include/playrender.h) computes, written from the header's rule and not from
the kernels, for the tests to compare against bit for bit.  Nothing here imports the package.

Input: G meshes packed as the mesher leaves them - ``vertices (V, 3)`` fp32, optional ``normals (V, 3)``, ``triangles (T, 3)`` int32
local to their group, ``vertex_offsets`` / ``triangle_offsets (G + 1)`` - and a cluster grid ``origin[3]``, ``cell[3]``, ``cells[3]``.
Per axis in fp32: ``q = (v - origin) / cell``, 0 unless ``q >= 0``, ``cells`` if ``q > cells``; ``c = min(int(q), cells - 1)``;
``w = q - c``; ``f = int(w 2^20)``.  Per (group, cell): the member count n and the int64 sums F; one output vertex per occupied cell in
flat-cell order at ``origin + (c + F / (n 2^20)) cell`` in fp64, rounded to fp32.  Normals: int64 sums of ``rint(x 2^20)`` over the
components with ``|x| <= 4``, normalised in fp64.  Triangles: out-of-range ones are dropped and counted, corners become cluster
indices, triangles with two equal corners are dropped, the rest are rotated to smallest-first and - unless duplicates are kept - only
the first of every rotated triple survives, in input order.
"""
import numpy as np

SCALE = 1048576          # 2^20


def lattice_grid(axes, k):
    """The cluster grid aligned with a lattice: per axis ``origin = x[0]``, ``cell = k (x[-1] - x[0]) / (n - 1)`` (in double, then
    rounded to fp32), ``cells = ceil((n - 1) / k)``."""
    origin = [float(np.float32(a[0])) for a in axes]
    cell = [float(np.float32(k * (float(np.float32(a[-1])) - float(np.float32(a[0]))) / (len(a) - 1))) for a in axes]
    cells = [-(-(len(a) - 1) // k) for a in axes]
    return origin, cell, cells


def vertex_cells(v, origin, cell, cells):
    """``(flat cell (V,), c (V, 3), f (V, 3))`` of vertices ``v (V, 3)`` fp32."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    origin, cell = np.asarray(origin, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    cells = np.asarray(cells, dtype=np.int64)
    top = cells.astype(np.float32)
    with np.errstate(all="ignore"):
        q = ((v - origin) / cell).astype(np.float32)
        q = np.where(q >= 0, q, np.float32(0))
        q = np.where(q > top, top, q).astype(np.float32)
        c = np.minimum(q.astype(np.int64), cells - 1)
        w = (q - c.astype(np.float32)).astype(np.float32)
        f = (w * np.float32(SCALE)).astype(np.float32).astype(np.int64)
    flat = (c[:, 0] * cells[1] + c[:, 1]) * cells[2] + c[:, 2]
    return flat, c, f


def _simplify_group(v, n, t, origin, cell, cells, keep_duplicates):
    V = len(v)
    flat, c, f = vertex_cells(v, origin, cell, cells)
    occupied, vertex_map = np.unique(flat, return_inverse=True)
    vertex_map = vertex_map.reshape(-1)
    K = len(occupied)
    members = np.bincount(vertex_map, minlength=K).astype(np.int64)
    F = np.zeros((K, 3), dtype=np.int64)
    np.add.at(F, vertex_map, f)
    cells64 = np.asarray(cells, dtype=np.int64)
    cc = np.stack([occupied // (cells64[1] * cells64[2]), (occupied // cells64[2]) % cells64[1], occupied % cells64[2]], axis=1)
    o64 = np.asarray(origin, dtype=np.float32).astype(np.float64)
    s64 = np.asarray(cell, dtype=np.float32).astype(np.float64)
    mean = F.astype(np.float64) / (members.astype(np.float64) * float(SCALE))[:, None]
    out_v = (o64 + (cc.astype(np.float64) + mean) * s64).astype(np.float32).reshape(-1, 3)
    out_n = None
    if n is not None:
        x = np.asarray(n, dtype=np.float32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            ok = np.abs(x) <= 4
            k = np.rint(np.where(ok, x, np.float32(0)) * np.float32(SCALE)).astype(np.int64)
        S = np.zeros((K, 3), dtype=np.int64)
        np.add.at(S, vertex_map, k)
        S = S.astype(np.float64)
        length = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        out_n = np.where(length[:, None] == 0, 0.0, S / np.where(length == 0, 1.0, length)[:, None]).astype(np.float32).reshape(-1, 3)
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    inside = np.all((t >= 0) & (t < V), axis=1)
    mapped = vertex_map[t[inside]].reshape(-1, 3).astype(np.int64)
    proper = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    mapped = mapped[proper]
    first = np.argmin(mapped, axis=1)
    rotated = np.take_along_axis(mapped, (first[:, None] + np.arange(3)) % 3, axis=1)
    if not keep_duplicates and len(rotated):
        key = rotated[:, 0] | rotated[:, 1] << 21 | rotated[:, 2] << 42
        _, lowest = np.unique(key, return_index=True)
        rotated = rotated[np.sort(lowest)]
    counts = [K, int(proper.sum()), len(rotated), int((~inside).sum())]
    return out_v, out_n, rotated.astype(np.int32).reshape(-1, 3), vertex_map.astype(np.int32), counts


def simplify(vertices, triangles, vertex_offsets, triangle_offsets, origin, cell, cells, normals=None, keep_duplicates=False):
    """Returns a dict: ``vertices``, ``normals`` (or None), ``triangles``, ``vertex_offsets``, ``triangle_offsets``, ``vertex_map (V)``
    int32 and ``counts (G, 4)`` int32 = clusters, non-degenerate triangles, output triangles, triangles with an index out of range."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    assert all(int(n) >= 1 for n in cells) and int(cells[0]) * int(cells[1]) * int(cells[2]) <= 1 << 21
    vo, to = [int(x) for x in vertex_offsets], [int(x) for x in triangle_offsets]
    parts = []
    for g in range(len(vo) - 1):
        n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)[vo[g]:vo[g + 1]]
        parts.append(_simplify_group(vertices[vo[g]:vo[g + 1]], n, triangles[to[g]:to[g + 1]], origin, cell, cells, keep_duplicates))
    return {
        "vertices": np.concatenate([p[0] for p in parts]).reshape(-1, 3),
        "normals": None if normals is None else np.concatenate([p[1] for p in parts]).reshape(-1, 3),
        "triangles": np.concatenate([p[2] for p in parts]).reshape(-1, 3),
        "vertex_offsets": np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int32),
        "triangle_offsets": np.concatenate([[0], np.cumsum([len(p[2]) for p in parts])]).astype(np.int32),
        "vertex_map": np.concatenate([p[3] for p in parts]).astype(np.int32),
        "counts": np.array([p[4] for p in parts], dtype=np.int32).reshape(-1, 4),
    }


def simplify_mesh(mesh, origin, cell, cells, keep_duplicates=False, normals=True):
    """``simplify`` of a ``surface_reference.extract_surface`` result (a dict)."""
    return simplify(mesh["vertices"], mesh["triangles"], mesh["vertex_offsets"], mesh["triangle_offsets"], origin, cell, cells,
                    normals=mesh["normals"] if normals else None, keep_duplicates=keep_duplicates)


# ------------------------------------------------------------------------------------------------ mesh properties (for the tests)
def directed_edges_balanced(triangles):
    """True iff every directed edge occurs exactly as often as its reverse: the triangles form a cycle (a closed oriented mesh, and
    every simplicial image of one)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if not len(t):
        return True
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    m = int(t.max()) + 1
    forward, fc = np.unique(e[:, 0] * m + e[:, 1], return_counts=True)
    backward, bc = np.unique(e[:, 1] * m + e[:, 0], return_counts=True)
    return bool(np.array_equal(forward, backward) and np.array_equal(fc, bc))

"""Closest-hit ray queries restated in numpy fp32 as an exhaustive search (not a test).

An independent statement of what ``pr_raycast_query`` (include/playrender.h) returns: every ray of a group is tested against every
triangle of the group with the header's fp32 formulas in the header's order, and the lexicographic minimum of (t, triangle index)
is taken.  There is no grid here - the GPU tests check that the grid changes nothing.  ``hit_point_error`` is a float64 check of the
hits for the property tests; ``grid_lists`` restates the build's lists (it is not used by the search).  Nothing here imports the
package.
"""
import numpy as np

F = np.float32
PAD = F(0.0625)
SLIVER = F(2.0 ** -20)


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def clamped_offsets(offsets, total):
    """Offsets that leave [0, total] or decrease are clamped (the header's rule)."""
    out, at = [], 0
    for x in np.asarray(offsets).tolist():
        at = min(int(total), max(at, int(x)))
        out.append(at)
    return out


def group_slices(mesh):
    """Per group: (vertices (V_g, 3), triangles (T_g, 3)) of the clamped slices."""
    v = np.ascontiguousarray(mesh["vertices"], dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(mesh["triangles"], dtype=np.int32).reshape(-1, 3)
    V, T = int(mesh.get("V", len(v))), int(mesh.get("T", len(t)))
    vo, to = clamped_offsets(mesh["vertex_offsets"], V), clamped_offsets(mesh["triangle_offsets"], T)
    return [(v[vo[g]:vo[g + 1]], t[to[g]:to[g + 1]]) for g in range(len(vo) - 1)]


def ray_triangle_tests(vertices, triangles, origins, directions, t_min, t_max, cull_back):
    """All rays (n, 3) against all triangles (T, 3) of one group: (accepted (n, T) bool, t, u, v (n, T) fp32, det (n, T))."""
    n, T = len(origins), len(triangles)
    valid = np.all((triangles >= 0) & (triangles < len(vertices)), axis=1) if len(vertices) else np.zeros(T, dtype=bool)
    if not valid.any():
        z = np.zeros((n, T), dtype=F)
        return np.zeros((n, T), dtype=bool), z, z, z, z
    tri = np.where(valid[:, None], triangles, 0)
    a, b, c = vertices[tri[:, 0]][None], vertices[tri[:, 1]][None], vertices[tri[:, 2]][None]
    o, d = origins[:, None, :], directions[:, None, :]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        p = cross(np.broadcast_to(d, (n, T, 3)), np.broadcast_to(e2, (n, T, 3)))
        det = dot(e1, p)
        s = o - a
        u = dot(s, p) / det
        q = cross(s, np.broadcast_to(e1, (n, T, 3)))
        v = dot(d, q) / det
        t = dot(e2, q) / det
        facing = (det > 0) if cull_back else ((det > 0) | (det < 0))
        accepted = facing & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= F(t_min)) & (t <= F(t_max)) & valid[None]
    assert t.dtype == F and u.dtype == F
    return accepted, t, u, v, det


def cast(mesh, origins, directions, t_min=0.0, t_max=np.inf, cull_back=False, pairs=1 << 21):
    """``mesh``: the packed dict of tests/surface_reference.py (``V`` / ``T``: the totals the call is told, default: the rows);
    ``origins`` / ``directions (G, N, 3)``.  Returns ``t (G, N)`` fp32 (+inf: miss), ``triangle (G, N)`` int32 (-1), ``barycentric
    (G, N, 2)`` (zeros), and for the property tests ``accepted (G, N)`` - how many triangles accept the ray -, ``ties (G, N)`` - how
    many of them at the smallest t - and ``det (G, N)`` of the winner (0 for a miss)."""
    origins, directions = np.asarray(origins, dtype=F), np.asarray(directions, dtype=F)
    G, N = origins.shape[:2]
    groups = group_slices(mesh)
    assert len(groups) == G and directions.shape == origins.shape == (G, N, 3)
    out = {"t": np.full((G, N), np.inf, dtype=F), "triangle": np.full((G, N), -1, dtype=np.int32),
           "barycentric": np.zeros((G, N, 2), dtype=F), "accepted": np.zeros((G, N), dtype=np.int64),
           "ties": np.zeros((G, N), dtype=np.int64), "det": np.zeros((G, N), dtype=F)}
    for g, (vertices, triangles) in enumerate(groups):
        if len(triangles) == 0 or N == 0:
            continue
        rows = max(1, pairs // len(triangles))
        for r0 in range(0, N, rows):
            sl = slice(r0, min(N, r0 + rows))
            accepted, t, u, v, det = ray_triangle_tests(vertices, triangles, origins[g, sl], directions[g, sl], t_min, t_max, cull_back)
            masked = np.where(accepted, t, F(np.inf))
            least = masked.min(axis=1)
            at_least = accepted & (t == least[:, None])
            hit = accepted.any(axis=1)
            index = np.argmax(at_least, axis=1)                       # the lowest index among equal t
            pick = lambda x: x[np.arange(len(index)), index]
            out["t"][g, sl] = np.where(hit, pick(t), F(np.inf))
            out["triangle"][g, sl] = np.where(hit, index, -1)
            out["barycentric"][g, sl, 0] = np.where(hit, pick(u), F(0))
            out["barycentric"][g, sl, 1] = np.where(hit, pick(v), F(0))
            out["det"][g, sl] = np.where(hit, pick(det), F(0))
            out["accepted"][g, sl] = accepted.sum(axis=1)
            out["ties"][g, sl] = at_least.sum(axis=1)
    return out


def hit_point_error(mesh, origins, directions, result):
    """Float64: per ray the distance between ``o + t d`` and ``a + u (b - a) + v (c - a)`` of the reported hit (0 for a miss), and the
    radius ``|o + t d|`` (nan for a miss) - an independent check that a reported hit is a point of its triangle on the ray."""
    G, N = result["t"].shape
    error, radius = np.zeros((G, N)), np.full((G, N), np.nan)
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        hit = result["triangle"][g] >= 0
        tri = triangles[result["triangle"][g][hit]]
        a, b, c = (vertices[tri[:, k]].astype(np.float64) for k in range(3))
        u, v = result["barycentric"][g][hit].astype(np.float64).T
        on_ray = origins[g][hit].astype(np.float64) + result["t"][g][hit].astype(np.float64)[:, None] * directions[g][hit].astype(np.float64)
        on_triangle = a + u[:, None] * (b - a) + v[:, None] * (c - a)
        error[g][hit] = np.linalg.norm(on_ray - on_triangle, axis=1)
        radius[g][hit] = np.linalg.norm(on_ray, axis=1)
    return error, radius


# ------------------------------------------------------------------------------------------------ the build's lists
def classify(vertices, triangles, origin, cell, cells):
    """The header's classification of every triangle of one group, in fp32: ``kind (T)`` = 0 dead, 1 loose, 2 tight, and the
    inclusive cell ranges ``lo``, ``hi (T, 3)`` of the tight ones."""
    origin, cell, top = np.asarray(origin, dtype=F), np.asarray(cell, dtype=F), np.asarray(cells, dtype=F)
    T = len(triangles)
    kind, lo, hi = np.zeros(T, dtype=np.int64), np.zeros((T, 3), dtype=np.int64), np.zeros((T, 3), dtype=np.int64)
    valid = np.all((triangles >= 0) & (triangles < len(vertices)), axis=1) if len(vertices) else np.zeros(T, dtype=bool)
    if not valid.any():
        return kind, lo, hi
    tri = np.where(valid[:, None], triangles, 0)
    a, b, c = vertices[tri[:, 0]], vertices[tri[:, 1]], vertices[tri[:, 2]]
    with np.errstate(all="ignore"):
        dead = ~valid | np.all(a == b, axis=1) | np.all(a == c, axis=1)
        e1, e2 = b - a, c - a
        n = cross(e1, e2)
        shaped = dot(n, n) > SLIVER * (dot(e1, e1) * dot(e2, e2))
        g = (np.stack([a, b, c], axis=1) - origin) / cell                        # (T, 3 corners, 3 axes)
        low, high = g.min(axis=1) - PAD, g.max(axis=1) + PAD
        inside = np.isfinite(g).all(axis=(1, 2)) & (low >= 0).all(axis=1) & (high <= top).all(axis=1)
        tight = ~dead & shaped & inside
        lo[tight] = low[tight].astype(np.int64)
        hi[tight] = np.minimum(high[tight].astype(np.int64), np.asarray(cells, dtype=np.int64) - 1)
    kind[~dead] = 1
    kind[tight] = 2
    return kind, lo, hi


def grid_lists(mesh, origin, cell, cells):
    """The lists of ``pr_raycast_build``: per group a list of C + 1 sorted arrays of local triangle indices (the last is the loose
    list)."""
    C = int(cells[0]) * int(cells[1]) * int(cells[2])
    out = []
    for vertices, triangles in group_slices(mesh):
        kind, lo, hi = classify(vertices, triangles, origin, cell, cells)
        lists = [[] for _ in range(C + 1)]
        lists[C] = np.nonzero(kind == 1)[0].tolist()
        for k in np.nonzero(kind == 2)[0].tolist():
            for x in range(lo[k, 0], hi[k, 0] + 1):
                for y in range(lo[k, 1], hi[k, 1] + 1):
                    for z in range(lo[k, 2], hi[k, 2] + 1):
                        lists[(x * cells[1] + y) * cells[2] + z].append(k)
        out.append([np.asarray(l, dtype=np.int32) for l in lists])             # (ascending: the triangles were visited in order)
    return out


# ------------------------------------------------------------------------------------------------ ray sets the tests share
def sphere_origins(rng, n, radius=3.0):
    x = rng.normal(size=(n, 3))
    return (radius * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)


def ball_points(rng, n, radius=0.5):
    x = rng.normal(size=(n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (radius * x * rng.uniform(0, 1, (n, 1)) ** (1 / 3)).astype(F)

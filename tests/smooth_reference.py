"""Incidence lists, Laplacian / Taubin steps and vertex normals restated in numpy (not a test).

An independent statement of what ``pr_mesh_smooth`` (include/playrender.h) returns, written from the header's words and without
atomics: the lists come from a stable argsort of the corner array, the ordered sums are vectorised over the vertices with a loop over
the position in the list, and everything is computed in ``np.float32`` (numpy rounds every operation on its own: no contraction).
Nothing here imports the package, and nothing but numpy is used.
"""
import numpy as np

F = np.float32
COUNTS = 8
HAS_TRIANGLES, BORDER, PINNED, OVER_DEGREE, NOT_FINITE, MOVABLE = 1, 2, 4, 8, 16, 32
PIN_BORDER = 1


def clamped_offsets(offsets, total):
    """Offsets that leave [0, total] or decrease are clamped (the header's rule)."""
    out, at = [], 0
    for x in np.asarray(offsets).tolist():
        at = min(int(total), max(at, int(x)))
        out.append(at)
    return out


def incidence_lists(vertices, triangles):
    """One group: ``(valid (T) bool, k (V) int64, begin (V + 1) int64, entries (3 valid) int64, corner (3 valid) int64)`` - the lists
    of all vertices back to back, ascending inside a list, and the corner (0, 1, 2) at which the vertex sits in each entry's triangle."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    valid = np.zeros(T, dtype=bool)
    if V and T:
        valid = np.all((t >= 0) & (t < V), axis=1)
        valid &= (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
        safe = np.where(valid[:, None], t, 0)
        valid &= np.isfinite(v[safe].reshape(T, 9)).all(axis=1)
    rows = np.nonzero(valid)[0]
    corners = t[rows].reshape(-1)                                   # triangle after triangle, corner after corner
    order = np.argsort(corners, kind="stable")                      # by vertex; inside a vertex by triangle: ascending
    k = np.bincount(corners, minlength=V).astype(np.int64) if V else np.zeros(0, dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    return valid, k, begin, np.repeat(rows, 3)[order], np.tile(np.arange(3), len(rows))[order]


def _dense(k, begin, values, covered, fill=-1):
    """``(len(covered), max k)``: the list values of the covered vertices, ``fill`` behind a list's end."""
    width = int(k[covered].max()) if len(covered) else 0
    at = begin[covered][:, None] + np.arange(width)[None, :]
    inside = np.arange(width)[None, :] < k[covered][:, None]
    return np.where(inside, values[np.where(inside, at, 0)] if len(values) else fill, fill), inside


def smooth_group(vertices, triangles, pinned=None, steps=0, lam=0.5, mu=-0.53, max_degree=64, flags=PIN_BORDER, want_normals=True):
    """One group: a dict with ``vertices``, ``normals`` (V, 3) fp32, ``k`` (V), ``entries`` (the lists back to back), ``state`` (V)
    int32 and ``counts`` (8) int64."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    valid, k, begin, entries, corner = incidence_lists(v, t)
    finite = np.isfinite(v).all(axis=1) if V else np.zeros(0, dtype=bool)
    listed = (k >= 1) & (k <= max_degree)
    covered = np.nonzero(listed)[0]
    # the others of every entry: (b, c), (c, a), (a, b) for the corner 0, 1, 2
    x = t[entries, (corner + 1) % 3] if len(entries) else np.zeros(0, dtype=np.int64)
    y = t[entries, (corner + 2) % 3] if len(entries) else np.zeros(0, dtype=np.int64)
    # border: some vertex occurs exactly once among the 2 k others of a listed vertex
    owner = np.repeat(np.arange(V), k)
    keys = np.concatenate([owner * max(V, 1) + x, owner * max(V, 1) + y])
    unique, occurrences = np.unique(keys, return_counts=True)
    border = np.zeros(V, dtype=bool)
    border[unique[occurrences == 1] // max(V, 1)] = True
    border &= listed
    pin = np.zeros(V, dtype=bool) if pinned is None else np.asarray(pinned).reshape(-1)[:V] != 0
    movable = finite & listed & ~pin & ~(border & bool(flags & PIN_BORDER))
    state = (np.where(k >= 1, HAS_TRIANGLES, 0) | np.where(border, BORDER, 0) | np.where(pin, PINNED, 0) |
             np.where(k > max_degree, OVER_DEGREE, 0) | np.where(finite, 0, NOT_FINITE) | np.where(movable, MOVABLE, 0)).astype(np.int32)
    # the steps: Jacobi, the sum over q_1 .. q_2k in order, one list position after the other
    moving = np.nonzero(movable)[0]
    X, inside = _dense(k, begin, x, moving)
    Y, _ = _dense(k, begin, y, moving)
    p = v.copy()
    with np.errstate(all="ignore"):
        for step in range(steps):
            f = F(lam) if step % 2 == 0 else F(mu)
            acc = np.zeros((len(moving), 3), dtype=F)
            for j in range(X.shape[1]):
                rows = np.nonzero(inside[:, j])[0]
                if j == 0:
                    acc[rows] = p[X[rows, 0]]
                else:
                    acc[rows] = acc[rows] + p[X[rows, j]]
                acc[rows] = acc[rows] + p[Y[rows, j]]
            mean = acc / (2 * k[moving]).astype(F)[:, None]
            new = p.copy()
            new[moving] = p[moving] + f * (mean - p[moving])
            p = new
    assert p.dtype == F
    normals = np.zeros((V, 3), dtype=F)
    if want_normals and len(covered):
        L, inside = _dense(k, begin, entries, covered)
        N = np.zeros((len(covered), 3), dtype=F)
        with np.errstate(all="ignore"):
            for j in range(L.shape[1]):
                rows = np.nonzero(inside[:, j])[0]
                tri = t[L[rows, j]]
                a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
                e1, e2 = b - a, c - a
                n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                              e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
                N[rows] = n if j == 0 else N[rows] + n
            length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
            good = np.isfinite(length) & (length > 0)
            normals[covered[good]] = N[good] / length[good][:, None]
        assert N.dtype == F and length.dtype == F
    counts = np.array([valid.sum(), T - valid.sum(), movable.sum(), (finite & (k == 0)).sum(), border.sum(), (k > max_degree).sum(),
                       (~finite).sum(), k.max() if V else 0], dtype=np.int64)
    return {"vertices": p, "normals": normals, "k": k, "entries": entries.astype(np.int32), "state": state, "counts": counts}


def smooth(mesh, pinned=None, steps=0, lam=0.5, mu=-0.53, max_degree=64, flags=PIN_BORDER):
    """``mesh``: the packed dict of tests/surface_reference.py (optionally with the totals ``V`` / ``T``); ``pinned (V)`` optional.
    Returns a dict: ``vertices``, ``normals (V, 3)`` fp32, ``incidence_offsets (V + 1)``, ``incidence (total)`` int32 - the written
    entries only -, ``state (V)`` int32 (-1 in the rows that no clamped group owns), ``counts (G, 8)`` int32 and ``k (V)``."""
    v = np.ascontiguousarray(mesh["vertices"], dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(mesh["triangles"], dtype=np.int32).reshape(-1, 3)
    V, T = int(mesh.get("V", len(v))), int(mesh.get("T", len(t)))
    vo, to = clamped_offsets(mesh["vertex_offsets"], V), clamped_offsets(mesh["triangle_offsets"], T)
    out_v = np.zeros((V, 3), dtype=F)
    out_v[:min(len(v), V)] = v[:V]
    out = {"vertices": out_v, "normals": np.zeros((V, 3), dtype=F), "state": np.full(V, -1, dtype=np.int32), "k": np.zeros(V, dtype=np.int64)}
    offsets, entries, counts, total = np.zeros(V + 1, dtype=np.int64), [], [], 0
    for g in range(len(vo) - 1):
        mask = None if pinned is None else np.asarray(pinned).reshape(-1)[vo[g]:vo[g + 1]]
        part = smooth_group(v[vo[g]:vo[g + 1]], t[to[g]:to[g + 1]], mask, steps, lam, mu, max_degree, flags)
        out["vertices"][vo[g]:vo[g + 1]] = part["vertices"]
        out["normals"][vo[g]:vo[g + 1]] = part["normals"]
        out["state"][vo[g]:vo[g + 1]] = part["state"]
        out["k"][vo[g]:vo[g + 1]] = part["k"]
        offsets[vo[g]:vo[g + 1]] = total + np.concatenate([[0], np.cumsum(part["k"])])[:-1]
        total += int(part["k"].sum())
        entries.append(part["entries"])
        counts.append(part["counts"])
    offsets[vo[-1]:] = total                                        # (the rows in front of the first group keep 0)
    out["incidence_offsets"] = offsets.astype(np.int32)
    out["incidence"] = np.concatenate(entries).astype(np.int32) if entries else np.zeros(0, dtype=np.int32)
    out["counts"] = np.stack(counts).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hand-made meshes
def single(vertices, triangles):
    return {"vertices": np.asarray(vertices, dtype=F).reshape(-1, 3), "triangles": np.asarray(triangles, dtype=np.int32).reshape(-1, 3),
            "vertex_offsets": np.array([0, len(vertices)], dtype=np.int32), "triangle_offsets": np.array([0, len(triangles)], dtype=np.int32)}


def tetrahedron():
    return single([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def one_triangle():
    return single([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def fan(n, closed=True):
    """A hub (vertex 0, lifted) with ``n`` rim vertices on the unit circle; ``closed``: n triangles around the hub, else n - 1."""
    angle = 2 * np.pi * np.arange(n) / n
    vertices = np.concatenate([[[0, 0, 0.5]], np.stack([np.cos(angle), np.sin(angle), np.zeros(n)], axis=1)]).astype(F)
    triangles = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n if closed else n - 1)]
    return single(vertices, triangles)


def broken():
    """The tetrahedron with two more triangles - one with a repeated index, one with a NaN corner - and the NaN vertex."""
    mesh = tetrahedron()
    vertices = np.concatenate([mesh["vertices"], [[np.nan, 0, 0]]]).astype(F)
    triangles = np.concatenate([mesh["triangles"], [[0, 1, 1], [0, 1, 4]]]).astype(np.int32)
    return single(vertices, triangles)

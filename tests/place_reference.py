"""Placement of simplified meshes' vertices by quadric error, restated in numpy (not a test).

An independent statement of what ``pr_mesh_place`` (include/playrender.h) computes, written from the header's rule and not from the
kernels, for the tests to compare against bit for bit.  Nothing here imports the package.

Per valid input triangle (three indices in ``[0, V_g)``, nine finite coordinates) and per distinct cluster ``j`` among
``vertex_map`` of its corners (entries outside ``[0, VO_g)`` contribute nothing), with ``m`` the stored merged vertex ``j`` in fp64:
``a' = (a - m) / h`` ..., ``n = (b' - a') x (c' - a')``, ``L = |n|``, ``d = -n . a'``; the nine coefficients ``n_i n_j / L`` and
``d n_i / L``; a contribution with ``L`` not finite or not > 0, or with a coefficient above ``2^16`` in magnitude or not finite, is
skipped and counted; otherwise ``rint(q 2^36)`` goes into nine int64 sums (modulo 2^64).  Per merged vertex with a contribution:
``M = A + lambda I`` with ``lambda = regularisation trace(A) / 3``, the adjugate solve in the header's order of operations, the vertex
moves by ``t = h y`` unless ``det`` is not finite or not > 0, a ``y_k`` is not finite or ``|t_k| > max_move_k``.  numpy rounds every
elementwise fp64 operation on its own, and its square root and division are correctly rounded: the header's arithmetic.
"""
import numpy as np

QUANTUM = float(2 ** 36)
LIMIT = float(2 ** 16)
COUNTS = 4


def clamp_offsets(offsets, total):
    """Offsets that leave ``[0, total]`` or decrease are clamped (the running maximum, cut at the total)."""
    out, at = [], 0
    for x in np.asarray(offsets, dtype=np.int64).reshape(-1):
        at = min(int(total), max(at, int(x)))
        out.append(at)
    return out


def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def _normals(v, t):
    v = v.astype(np.float64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return _cross(b - a, c - a)


def quadric_sums(v, t, vmap, m, h):
    """``(sums (VO, 9) int64, contributions (VO) int64, bad)`` of one group: ``v (V, 3)`` / ``m (VO, 3)`` fp32, ``t (T, 3)``,
    ``vmap (V)``; ``bad`` = invalid triangles + skipped contributions."""
    V, VO = len(v), len(m)
    sums, contributions = np.zeros((VO, 9), dtype=np.int64), np.zeros(VO, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    in_range = np.all((t >= 0) & (t < V), axis=1)
    finite = np.zeros(len(t), dtype=bool)
    finite[in_range] = np.isfinite(v[t[in_range]].astype(np.float64)).all(axis=(1, 2))
    valid = in_range & finite
    bad = int((~valid).sum())
    t = t[valid]
    if not len(t) or not VO:
        return sums, contributions, bad
    j = vmap[t].astype(np.int64)                                       # (n, 3)
    reach = (j >= 0) & (j < VO)
    corners = v[t].astype(np.float64)                                  # (n, 3 corners, 3 axes)
    m64 = m.astype(np.float64)
    for e in range(3):
        first = reach[:, e].copy()                                     # distinct: no earlier corner has the same cluster
        for before in range(e):
            first &= j[:, before] != j[:, e]
        rows, cluster = np.flatnonzero(first), j[first, e]
        if not len(rows):
            continue
        with np.errstate(all="ignore"):
            centre = m64[cluster]
            a, b, c = ((corners[rows, k] - centre) / h for k in range(3))
            n = _cross(b - a, c - a)
            L = np.sqrt(_dot(n, n))
            d = -_dot(n, a)
            q = np.stack([n[:, 0] * n[:, 0] / L, n[:, 0] * n[:, 1] / L, n[:, 0] * n[:, 2] / L, n[:, 1] * n[:, 1] / L,
                          n[:, 1] * n[:, 2] / L, n[:, 2] * n[:, 2] / L, d * n[:, 0] / L, d * n[:, 1] / L, d * n[:, 2] / L], axis=1)
            good = np.isfinite(L) & (L > 0) & (np.abs(q) <= LIMIT).all(axis=1)          # (a NaN fails the comparison)
        bad += int((~good).sum())
        k = np.rint(q[good] * QUANTUM).astype(np.int64)
        np.add.at(sums, cluster[good], k)                              # (int64 wraps: modulo 2^64)
        np.add.at(contributions, cluster[good], 1)
    return sums, contributions, bad


def solve(sums, contributions, m, h, max_move, regularisation):
    """``(out (VO, 3) fp32, moved (VO) bool)`` from the sums of one group."""
    m = np.asarray(m, dtype=np.float32).reshape(-1, 3)
    S = sums.astype(np.float64) * (1.0 / QUANTUM)
    with np.errstate(all="ignore"):
        lam = regularisation * ((S[:, 0] + S[:, 3]) + S[:, 5]) / 3.0
        m00, m01, m02, m11, m12, m22 = S[:, 0] + lam, S[:, 1], S[:, 2], S[:, 3] + lam, S[:, 4], S[:, 5] + lam
        r0, r1, r2 = -S[:, 6], -S[:, 7], -S[:, 8]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        y = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
        t = h * y
        moved = (contributions > 0) & np.isfinite(det) & (det > 0) & np.isfinite(y).all(axis=1) & \
            ~(np.abs(t) > np.asarray(max_move, dtype=np.float64)).any(axis=1)
        placed = (m.astype(np.float64) + t).astype(np.float32)
    out = m.copy()
    out[moved] = placed[moved]
    return out, moved


def place(vertices, triangles, vertex_offsets, triangle_offsets, vertex_map, merged_vertices, merged_vertex_offsets, *, scale, max_move,
          regularisation=2.0 ** -10, merged_triangles=None, merged_triangle_offsets=None, out=None):
    """Returns a dict: ``vertices (VO, 3)`` fp32 - ``out`` (default: a copy of the merged vertices) with the rows of the clamped
    groups written - and ``counts (G, 4)`` int32 = moved, kept, skipped contributions + invalid triangles, turned.  The host values
    enter as ``float(np.float32(x))``, as the library reads them from the description."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    vmap = np.asarray(vertex_map, dtype=np.int32).reshape(-1)
    m = np.asarray(merged_vertices, dtype=np.float32).reshape(-1, 3)
    h, reg = float(np.float32(scale)), float(np.float32(regularisation))
    move = [float(np.float32(x)) for x in max_move]
    vo, to, mo = clamp_offsets(vertex_offsets, len(v)), clamp_offsets(triangle_offsets, len(t)), clamp_offsets(merged_vertex_offsets, len(m))
    u = uo = None
    if merged_triangles is not None:
        u = np.asarray(merged_triangles, dtype=np.int32).reshape(-1, 3)
        uo = clamp_offsets(merged_triangle_offsets, len(u))
    G = len(vo) - 1
    result = m.copy() if out is None else np.array(out, dtype=np.float32).reshape(-1, 3)
    counts = np.zeros((G, COUNTS), dtype=np.int32)
    for g in range(G):
        mg = m[mo[g]:mo[g + 1]]
        sums, contributions, bad = quadric_sums(v[vo[g]:vo[g + 1]], t[to[g]:to[g + 1]], vmap[vo[g]:vo[g + 1]], mg, h)
        placed, moved = solve(sums, contributions, mg, h, move, reg)
        result.view(np.uint32)[mo[g]:mo[g + 1]] = placed.view(np.uint32)
        turned = 0
        if u is not None:
            ug = u[uo[g]:uo[g + 1]].astype(np.int64)
            ug = ug[np.all((ug >= 0) & (ug < len(mg)), axis=1)]
            if len(ug):
                with np.errstate(all="ignore"):
                    turned = int((_dot(_normals(mg, ug), _normals(placed, ug)) < 0).sum())
        counts[g] = [int(moved.sum()), len(mg) - int(moved.sum()), bad, turned]
    return {"vertices": result, "counts": counts}


def place_simplified(mesh, simplified, cell, *, max_move=None, regularisation=2.0 ** -10):
    """``place`` of a ``simplify_reference.simplify`` result ``simplified`` of the ``surface_reference.extract_surface`` result
    ``mesh`` as ``surface.simplify_meshes(placement="quadric")`` calls it: ``scale = max(cell)``, ``max_move = cell``."""
    return place(mesh["vertices"], mesh["triangles"], mesh["vertex_offsets"], mesh["triangle_offsets"], simplified["vertex_map"],
                 simplified["vertices"], simplified["vertex_offsets"], scale=max(cell), max_move=cell if max_move is None else max_move,
                 regularisation=regularisation, merged_triangles=simplified["triangles"],
                 merged_triangle_offsets=simplified["triangle_offsets"])


# ------------------------------------------------------------------------------------------------ fields and measures (for the tests)
def box_field(n, half=(0.53, 0.41, 0.37), rz=0.0, rx=0.0):
    """``-max(|x| - 0.53, |y| - 0.41, |z| - 0.37)`` on ``linspace(-1, 1, n)``, the box rotated by ``rz`` about z, then ``rx`` about x."""
    a = np.linspace(-1, 1, n)
    p = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1)
    cz, sz, cx, sx = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    q = p @ R                                                          # the point in the box's frame: R^T p
    s = -np.max(np.abs(q) - np.asarray(half), axis=-1)
    return s.astype(np.float32), [a.astype(np.float32)] * 3, R


def box_distance(points, half=(0.53, 0.41, 0.37), R=None):
    """Unsigned distance of ``points (N, 3)`` to the surface of the box."""
    q = np.asarray(points, dtype=np.float64) @ (np.eye(3) if R is None else R)
    e = np.abs(q) - np.asarray(half)
    outside = np.linalg.norm(np.maximum(e, 0), axis=1)
    return np.where((e <= 0).all(axis=1), -e.max(axis=1), outside)


def volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6)


def doubled_areas(vertices, triangles):
    return np.linalg.norm(_normals(np.asarray(vertices, dtype=np.float32), np.asarray(triangles, dtype=np.int64)), axis=1)

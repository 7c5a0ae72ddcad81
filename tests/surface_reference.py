"""Marching tetrahedra on the Freudenthal (Kuhn) split of a rectilinear lattice, restated in numpy (not a test).

An independent statement of what ``pr_extract_surface`` (include/playrender.h) computes, for the tests to compare against bit for
bit: it derives its own case table from the orientation rule, emits vertices and triangles in the canonical order and does the
fp32 arithmetic in the stated order.  Nothing here imports the package.

Lattice: ``sigma (G, nx, ny, nz)`` fp32, z fastest; point (i, j, k) sits at (x[i], y[j], z[k]).  INSIDE iff ``sigma > level`` (a NaN
is never inside).  Seven edge directions leave a point, ``DIRECTIONS[d]``; an edge crosses when exactly one end is inside and then
carries one vertex, computed from its LOWER end a and far end b: ``t = (level - s_a) / (s_b - s_a)``, 0 unless ``t >= 0``, 1 if
``t > 1``, ``v = p_a + t (p_b - p_a)``.  A cube has six tetrahedra, one per axis permutation (``PERMUTATIONS``): corners
``0, e_p0, e_p0 + e_p1, (1, 1, 1)``.  Vertices are ordered by group, flat lower end, d; triangles by group, flat cube origin,
tetrahedron, triangle of the table row; indices are local to the group.
"""
import itertools

import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations(range(3)))          # lexicographic: (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)


def tetrahedron_corners(perm):
    """The four corners of the tetrahedron of axis permutation ``perm`` on the unit cube, as integer (3,) arrays."""
    e = np.eye(3, dtype=np.int64)
    v1 = e[perm[0]]
    return [np.zeros(3, dtype=np.int64), v1, v1 + e[perm[1]], np.ones(3, dtype=np.int64)]


def case_rows(perm):
    """``rows[mask]`` = list of triangles of the tetrahedron for the case ``mask`` (bit i = corner i inside); a triangle is three
    edges ``(i, j)``, i < j, of tetrahedron corners.  Orientation: with every crossing at its edge midpoint the triangle normal has
    a positive dot product with ``|inside| sum(outside corners) - |outside| sum(inside corners)`` (integers throughout)."""
    corners = tetrahedron_corners(perm)
    rows = []
    for mask in range(16):
        inside = [i for i in range(4) if mask >> i & 1]
        outside = [i for i in range(4) if not mask >> i & 1]
        edge = lambda a, b: (min(a, b), max(a, b))
        if len(inside) in (0, 4):
            triangles = []
        elif len(inside) == 1 or len(inside) == 3:
            lone = inside[0] if len(inside) == 1 else outside[0]
            triangles = [[edge(lone, b) for b in range(4) if b != lone]]
        else:
            (a, b), (c, d) = inside, outside
            q = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
            triangles = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
        outward = len(inside) * sum(corners[i] for i in outside) - len(outside) * sum(corners[i] for i in inside) if triangles else None
        fixed = []
        for tri in triangles:
            p = [corners[i] + corners[j] for i, j in tri]               # twice the edge midpoints
            dot = int(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), outward))
            assert dot != 0
            fixed.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
        rows.append(fixed)
    return rows


def _direction_index(delta):
    return DIRECTIONS.index(tuple(int(v) for v in delta))


def lookup_tables():
    """The table as arrays: ``count (6, 16)``, and per (tetrahedron, case, triangle, entry) the cube corner offset of the edge's lower
    end ``lower (6, 16, 2, 3, 3)`` and its direction ``direction (6, 16, 2, 3)``; ``corner (6, 4, 3)`` are the tetrahedron corners."""
    count = np.zeros((6, 16), dtype=np.int64)
    lower = np.zeros((6, 16, 2, 3, 3), dtype=np.int64)
    direction = np.zeros((6, 16, 2, 3), dtype=np.int64)
    corner = np.zeros((6, 4, 3), dtype=np.int64)
    for t, perm in enumerate(PERMUTATIONS):
        corners = tetrahedron_corners(perm)
        corner[t] = np.stack(corners)
        for mask, triangles in enumerate(case_rows(perm)):
            count[t, mask] = len(triangles)
            for s, tri in enumerate(triangles):
                for e, (i, j) in enumerate(tri):
                    lower[t, mask, s, e] = corners[i]
                    direction[t, mask, s, e] = _direction_index(corners[j] - corners[i])
    return count, lower, direction, corner


def lattice_gradient(s, axes):
    """``(nx, ny, nz, 3)`` fp32: per axis (s[i+1] - s[i-1]) / (x[i+1] - x[i-1]), one-sided at the two ends."""
    g = np.zeros(s.shape + (3,), dtype=np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            x = np.asarray(axes[a], dtype=np.float32)
            n = s.shape[a]
            hi = np.minimum(np.arange(n) + 1, n - 1)
            lo = np.maximum(np.arange(n) - 1, 0)
            ds = np.take(s, hi, axis=a) - np.take(s, lo, axis=a)
            dx = (x[hi] - x[lo]).reshape([-1 if b == a else 1 for b in range(3)])
            g[..., a] = ds / dx
    return g


def _extract_group(s, axes, level, normals, tables):
    count_lut, lower_lut, direction_lut, corner_lut = tables
    nx, ny, nz = s.shape
    level = np.float32(level)
    inside = s > level
    strides = np.array([ny * nz, nz, 1], dtype=np.int64)
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    index = np.stack([ii, jj, kk], axis=-1).reshape(-1, 3)
    P = nx * ny * nz
    top = np.array([nx, ny, nz]) - 1
    flat_inside = inside.reshape(-1)
    # crossing mask per point
    mask = np.zeros(P, dtype=np.int64)
    for d, delta in enumerate(DIRECTIONS):
        delta = np.array(delta)
        exists = np.all(index + delta <= top, axis=1)
        far = np.where(exists, index @ strides + delta @ strides, 0)
        mask |= (exists & (flat_inside != flat_inside[far])).astype(np.int64) << d
    bits = (mask[:, None] >> np.arange(7)) & 1
    base = np.concatenate([[0], np.cumsum(bits.sum(1))])[:-1]
    point, d = np.nonzero(bits)                                        # C order: by point, then d
    delta = np.array(DIRECTIONS)[d]
    a, b = index[point], index[point] + delta
    fs = s.reshape(-1)
    with np.errstate(all="ignore"):
        sa, sb = fs[a @ strides], fs[b @ strides]
        t = (level - sa) / (sb - sa)
        t = np.where(t >= 0, t, np.float32(0))
        t = np.where(t > 1, np.float32(1), t).astype(np.float32)
        vertices = np.zeros((len(point), 3), dtype=np.float32)
        for ax in range(3):
            x = np.asarray(axes[ax], dtype=np.float32)
            pa, pb = x[a[:, ax]], x[b[:, ax]]
            vertices[:, ax] = pa + t * (pb - pa)
        out_normals = None
        if normals:
            g = lattice_gradient(s, axes).reshape(-1, 3)
            ga, gb = g[a @ strides], g[b @ strides]
            n = -(ga + t[:, None] * (gb - ga))
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float32)
            ok = np.isfinite(length) & (length > 0)
            out_normals = np.where(ok[:, None], n / np.where(ok, length, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    # triangles, one tetrahedron at a time
    cube = np.all(index < top, axis=1)
    origin = index[cube]
    C = len(origin)
    valid = np.zeros((C, 6, 2), dtype=bool)
    ids = np.zeros((C, 6, 2, 3), dtype=np.int64)
    for t_idx in range(6):
        case = np.zeros(C, dtype=np.int64)
        for i in range(4):
            case |= flat_inside[(origin + corner_lut[t_idx, i]) @ strides].astype(np.int64) << i
        cnt = count_lut[t_idx, case]
        for slot in range(2):
            valid[:, t_idx, slot] = cnt > slot
            for e in range(3):
                low = (origin + lower_lut[t_idx, case, slot, e]) @ strides
                dd = direction_lut[t_idx, case, slot, e]
                below = mask[low] & ((1 << dd) - 1)
                ids[:, t_idx, slot, e] = base[low] + ((below[:, None] >> np.arange(7)) & 1).sum(1)
    triangles = ids[valid].astype(np.int32).reshape(-1, 3)
    return vertices, out_normals, triangles


def extract_surface(sigma, axes, level, normals=True):
    """``sigma (G, nx, ny, nz)``, ``axes`` = three coordinate arrays.  Returns a dict: ``vertices (V, 3)`` fp32, ``normals (V, 3)`` fp32
    or None, ``triangles (T, 3)`` int32 (local to the group), ``vertex_offsets`` / ``triangle_offsets (G + 1)`` int32."""
    sigma = np.asarray(sigma, dtype=np.float32)
    assert sigma.ndim == 4 and min(sigma.shape[1:]) >= 2
    tables = lookup_tables()
    parts = [_extract_group(sigma[g], axes, level, normals, tables) for g in range(sigma.shape[0])]
    return {
        "vertices": np.concatenate([p[0] for p in parts]).reshape(-1, 3),
        "normals": np.concatenate([p[1] for p in parts]).reshape(-1, 3) if normals else None,
        "triangles": np.concatenate([p[2] for p in parts]).reshape(-1, 3),
        "vertex_offsets": np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int32),
        "triangle_offsets": np.concatenate([[0], np.cumsum([len(p[2]) for p in parts])]).astype(np.int32),
    }


# ------------------------------------------------------------------------------------------------ mesh properties (for the tests)
def directed_edges_once(triangles):
    """True iff every directed edge occurs exactly once and its reverse exactly once: closed and consistently oriented."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = e[:, 0] * (t.max() + 1 if len(t) else 1) + e[:, 1]
    rev = e[:, 1] * (t.max() + 1 if len(t) else 1) + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool(np.all(counts == 1)) and bool(np.array_equal(np.sort(rev), uniq))


def euler_characteristic(vertex_count, triangles):
    t = np.asarray(triangles, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return int(vertex_count) - len(np.unique(e, axis=0)) + len(t)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def triangle_areas(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def triangle_normals(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])


# ------------------------------------------------------------------------------------------------ the fields the tests share
def sphere_field(n, r=0.63):
    x = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (r * r - X * X - Y * Y - Z * Z).astype(np.float32), [x.astype(np.float32)] * 3


def torus_field(n, R=0.55, a=0.23):
    x = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (a * a - (np.sqrt(X * X + Y * Y) - R) ** 2 - Z * Z).astype(np.float32), [x.astype(np.float32)] * 3


def plane_field():
    axes = [np.array([0, .1, .25, .7, 1]), np.linspace(-1, 1, 6), np.linspace(2, 3, 4)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return (0.3 * X - 0.2 * Y + 0.5 * Z).astype(np.float32), [a.astype(np.float32) for a in axes]

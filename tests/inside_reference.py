"""Inside / outside queries restated in numpy as an exhaustive sum (not a test).

An independent statement of what ``pr_inside_query`` (include/playrender.h) returns: every point of a group is tested against every
candidate triangle of the group with the header's rule, and the orientations of the triangles ahead of the point are summed.  There
is no grid in ``rule``.  The edge signs are exact: a float64 filter with a deliberately loose bound decides the clear cases, and every
other case - every zero among them - is evaluated in rational arithmetic (``fractions``).  ``coverage`` is the sum of the
orientations over ALL candidates, whether ahead or not: zero for every point of a mesh whose directed edges balance.  ``walk``
restates the kernel's column walk over ``raycast_reference.grid_lists`` with the once-per-column rule; that it equals ``rule`` is the
claim of DESIGN.md 23.2.  Nothing here imports the package.
"""
from fractions import Fraction

import numpy as np

from tests.raycast_reference import PAD, grid_lists, group_slices

F = np.float32
FILTER = 2.0 ** -50                  # looser than the kernel's bound on purpose: the two filters share nothing, the exact signs agree


def exact_edge_sign(ui, uj, vi, vj, pi, pj):
    """The header's s(u, v) for one edge, in rational arithmetic throughout."""
    ui, uj, vi, vj, pi, pj = (Fraction(float(x)) for x in (ui, uj, vi, vj, pi, pj))
    e = (vi - ui) * (pj - uj) - (vj - uj) * (pi - ui)
    if e != 0:
        return 1 if e > 0 else -1
    if uj != vj:
        return 1 if uj > vj else -1
    if vi != ui:
        return 1 if vi > ui else -1
    return 0


def edge_signs(u, v, p, counters=None):
    """``s(u, v)`` for rows of 2-D fp32 points ``u``, ``v``, ``p (M, 2)`` = (coordinate i, coordinate j): int64 ``(M)``."""
    u64, v64, p64 = u.astype(np.float64), v.astype(np.float64), p.astype(np.float64)
    left = (v64[:, 0] - u64[:, 0]) * (p64[:, 1] - u64[:, 1])
    right = (v64[:, 1] - u64[:, 1]) * (p64[:, 0] - u64[:, 0])
    det = left - right
    clear = np.abs(det) > FILTER * (np.abs(left) + np.abs(right))
    out = np.where(clear, np.sign(det), 0).astype(np.int64)
    rest = np.nonzero(~clear)[0]
    for m in rest.tolist():
        out[m] = exact_edge_sign(u[m, 0], u[m, 1], v[m, 0], v[m, 1], p[m, 0], p[m, 1])
    if counters is not None:
        counters["edges"] = counters.get("edges", 0) + len(out)
        counters["exact"] = counters.get("exact", 0) + len(rest)
        if len(rest):
            zero = [(Fraction(float(v[m, 0])) - Fraction(float(u[m, 0]))) * (Fraction(float(p[m, 1])) - Fraction(float(u[m, 1]))) ==
                    (Fraction(float(v[m, 1])) - Fraction(float(u[m, 1]))) * (Fraction(float(p[m, 0])) - Fraction(float(u[m, 0])))
                    for m in rest.tolist()]
            counters["zeros"] = counters.get("zeros", 0) + int(sum(zero))
    return out


def candidates(vertices, triangles):
    """``(candidate (T) bool, a, b, c (T, 3) fp32)``: not dead by the build's rule, nine finite coordinates."""
    T = len(triangles)
    valid = np.all((triangles >= 0) & (triangles < len(vertices)), axis=1) if len(vertices) and T else np.zeros(T, dtype=bool)
    tri = np.where(valid[:, None], triangles, 0)
    if not valid.any():
        z = np.zeros((T, 3), dtype=F)
        return valid, z, z, z
    a, b, c = vertices[tri[:, 0]], vertices[tri[:, 1]], vertices[tri[:, 2]]
    with np.errstate(all="ignore"):
        dead = ~valid | np.all(a == b, axis=1) | np.all(a == c, axis=1)
        finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    return ~dead & finite, a, b, c


def pair_rule(a, b, c, p, axis, counters=None):
    """The rule for rows of (triangle, point) pairs: ``(o (M), ahead (M) bool)``; ``o`` is the orientation whether ahead or not."""
    k = axis
    i, j = (k + 1) % 3, (k + 2) % 3
    ij = [i, j]
    sab = edge_signs(a[:, ij], b[:, ij], p[:, ij], counters)
    sbc = edge_signs(b[:, ij], c[:, ij], p[:, ij], counters)
    sca = edge_signs(c[:, ij], a[:, ij], p[:, ij], counters)
    o = np.where((sab == sbc) & (sbc == sca), sab, 0)
    a64, b64, c64, p64 = (x.astype(np.float64) for x in (a, b, c, p))
    e1, e2, d = b64 - a64, c64 - a64, p64 - a64
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    S = (n0 * d[:, 0] + n1 * d[:, 1]) + n2 * d[:, 2]
    above = np.maximum(np.maximum(a[:, k], b[:, k]), c[:, k]) > p[:, k]
    ahead = (o != 0) & above & (np.sign(S) == -o)
    return o, ahead


def _boxes(a, b, c, axis):
    i, j = (axis + 1) % 3, (axis + 2) % 3
    lo = np.minimum(np.minimum(a, b), c)
    hi = np.maximum(np.maximum(a, b), c)
    return lo[:, i], hi[:, i], lo[:, j], hi[:, j]


def rule(mesh, points, axis, reject=True, counters=None, rows=1 << 22):
    """``mesh``: the packed dict of tests/surface_reference.py; ``points (G, N, 3)``.  Returns ``winding``, ``crossings``, ``coverage
    (G, N)`` int32.  ``reject``: skip the pairs whose point lies strictly outside the triangle's closed (i, j) box - their orientation
    is 0 by the rule, so this only saves time (tests/test_inside_cpu.py checks that on a sample with ``reject=False``)."""
    points = np.asarray(points, dtype=F)
    G, N = points.shape[:2]
    groups = group_slices(mesh)
    assert len(groups) == G and points.shape == (G, N, 3)
    out = {key: np.zeros((G, N), dtype=np.int32) for key in ("winding", "crossings", "coverage")}
    i, j = (axis + 1) % 3, (axis + 2) % 3
    for g, (vertices, triangles) in enumerate(groups):
        if len(triangles) == 0 or N == 0:
            continue
        cand, a, b, c = candidates(vertices, triangles)
        if not cand.any():
            continue
        li, hi_, lj, hj = _boxes(a, b, c, axis)
        finite = np.isfinite(points[g]).all(axis=1)
        step = max(1, rows // len(triangles))
        for r0 in range(0, N, step):
            p = points[g, r0:r0 + step]
            with np.errstate(all="ignore"):
                pairs = cand[None, :] & finite[r0:r0 + step, None]
                if reject:
                    pairs = pairs & (p[:, None, i] >= li[None]) & (p[:, None, i] <= hi_[None]) & (p[:, None, j] >= lj[None]) & (p[:, None, j] <= hj[None])
            pi, ti = np.nonzero(pairs)
            if len(pi) == 0:
                continue
            o, ahead = pair_rule(a[ti], b[ti], c[ti], p[pi], axis, counters)
            np.add.at(out["coverage"][g], r0 + pi, o.astype(np.int32))
            np.add.at(out["winding"][g], r0 + pi, np.where(ahead, o, 0).astype(np.int32))
            np.add.at(out["crossings"][g], r0 + pi, ahead.astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ the kernel's walk restated
def walk(mesh, origin, cell, cells, points, axis, lists=None):
    """The column walk of ``k_inside_query`` over the build's lists: ``winding``, ``crossings (G, N)`` - equal to ``rule``'s, that is
    the claim under test - and ``cells_walked``, ``triangles_tested (G, N)``."""
    points = np.asarray(points, dtype=F)
    G, N = points.shape[:2]
    lists = grid_lists(mesh, origin, cell, cells) if lists is None else lists
    k = axis
    i, j = (k + 1) % 3, (k + 2) % 3
    C = int(cells[0]) * int(cells[1]) * int(cells[2])
    o32, c32 = np.asarray(origin, dtype=F), np.asarray(cell, dtype=F)
    out = {key: np.zeros((G, N), dtype=np.int32) for key in ("winding", "crossings")}
    out["cells_walked"] = np.zeros((G, N), dtype=np.int64)
    out["triangles_tested"] = np.zeros((G, N), dtype=np.int64)
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        if len(triangles) == 0:
            continue
        cand, a, b, c = candidates(vertices, triangles)
        with np.errstate(all="ignore"):                                 # the build's `low` on axis k, its own expression
            gk = (np.stack([a[:, k], b[:, k], c[:, k]], axis=1) - o32[k]) / c32[k]
            low = gk.min(axis=1) - PAD
        pairs_p, pairs_t = [], []
        for n in range(N):
            p = points[g, n]
            if not np.isfinite(p).all():
                continue
            members = [lists[g][C]]
            with np.errstate(all="ignore"):
                grid = (p - o32) / c32
            assert grid.dtype == F
            if grid[i] >= 0 and grid[i] < F(cells[i]) and grid[j] >= 0 and grid[j] < F(cells[j]) and grid[k] < F(cells[k]):
                at = [0, 0, 0]
                at[i], at[j] = int(grid[i]), int(grid[j])
                start = int(grid[k]) if grid[k] >= 0 else 0
                for m in range(start, cells[k]):
                    at[k] = m
                    listed = lists[g][(at[0] * cells[1] + at[1]) * cells[2] + at[2]]
                    out["cells_walked"][g, n] += 1
                    if len(listed):
                        lo = low[listed].astype(np.int64)
                        members.append(listed[np.maximum(lo, start) == m])
            members = np.concatenate(members).astype(np.int64)
            members = members[cand[members]]
            out["triangles_tested"][g, n] = len(members)
            pairs_p.append(np.full(len(members), n, dtype=np.int64))
            pairs_t.append(members)
        if not pairs_p:
            continue
        pi, ti = np.concatenate(pairs_p), np.concatenate(pairs_t)
        # the kernel's exact rejections, before the edges
        p = points[g][pi]
        li, hi_, lj, hj = _boxes(a[ti], b[ti], c[ti], axis)
        keep = (p[:, i] >= li) & (p[:, i] <= hi_) & (p[:, j] >= lj) & (p[:, j] <= hj) & (np.maximum(np.maximum(a[ti, k], b[ti, k]), c[ti, k]) > p[:, k])
        pi, ti = pi[keep], ti[keep]
        if len(pi) == 0:
            continue
        o, ahead = pair_rule(a[ti], b[ti], c[ti], points[g][pi], axis)
        np.add.at(out["winding"][g], pi, np.where(ahead, o, 0).astype(np.int32))
        np.add.at(out["crossings"][g], pi, ahead.astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ meshes and point sets the tests share
def directed_edges_balanced(mesh):
    """Whether in every group every directed edge - by vertex VALUES, over the candidates - occurs as often as its reverse."""
    for vertices, triangles in group_slices(mesh):
        cand, a, b, c = candidates(vertices, triangles)
        count = {}
        for u, v in ((a, b), (b, c), (c, a)):
            for x, y in zip(u[cand].view(np.int32).tolist(), v[cand].view(np.int32).tolist()):
                x, y = tuple(x), tuple(y)
                if x != y:
                    count[(x, y)] = count.get((x, y), 0) + 1
        if any(count.get((y, x), 0) != times for (x, y), times in count.items()):
            return False
    return True


def distance_from_mesh(mesh, points):
    """Float64 distance ``(G, N)`` of every point from its group's candidates (vectorised Ericson; inf without candidates)."""
    points = np.asarray(points, dtype=np.float64)
    G, N = points.shape[:2]
    out = np.full((G, N), np.inf)
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        cand, a, b, c = candidates(vertices, triangles)
        if not cand.any():
            continue
        a, b, c = (x[cand].astype(np.float64) for x in (a, b, c))
        for n in range(N):
            p = points[g, n]
            if not np.isfinite(p).all():
                continue
            ab, ac, ap = b - a, c - a, p - a
            d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
            d00, d01, d11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
            den = d00 * d11 - d01 * d01
            with np.errstate(all="ignore"):
                v = np.clip((d11 * d1 - d01 * d2) / den, 0, 1)
                w = np.clip((d00 * d2 - d01 * d1) / den, 0, 1)
            best = np.full(len(a), np.inf)
            inside = np.isfinite(v) & np.isfinite(w) & (v + w <= 1)
            q = a + v[:, None] * ab + w[:, None] * ac
            best[inside] = np.linalg.norm(p - q, axis=1)[inside]
            for u, e in ((a, b - a), (b, c - b), (c, a - c)):          # the three edges as segments
                with np.errstate(all="ignore"):
                    t = np.clip(((p - u) * e).sum(1) / (e * e).sum(1), 0, 1)
                t = np.where(np.isfinite(t), t, 0)
                best = np.minimum(best, np.linalg.norm(p - (u + t[:, None] * e), axis=1))
            out[g, n] = best.min()
    return out


SETS = ("uniform", "vertices", "below_above", "lattice", "midpoints", "faces", "corners", "outside", "far", "not_finite")


def point_batch(mesh, axes, n, grids, seed=0):
    """``(points (G, 10 n, 3), sets)``: the point sets of the tests, ``n`` points each (a multiple of 6), concatenated; ``sets`` names
    the slices.  Uniform in the lattice's box; ON mesh vertices (copies); exactly below and above vertices along each of the three
    axes (two coordinates copied); lattice points; edge midpoints; in cell faces and at cell corners of the two ``grids``; outside
    the first grid's box on each of its six sides (the other two coordinates inside it: below the grid along the ray's axis the whole
    column still counts); 2^12 cells of the first grid away along one axis, either side; a NaN or an infinite component."""
    assert n % 6 == 0
    rng = np.random.default_rng(300 + seed)
    low = np.array([float(a[0]) for a in axes])
    extent = np.array([float(a[-1]) - float(a[0]) for a in axes])
    all_p, sets = [], {}
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        parts, at = [], 0

        def add(name, p):
            nonlocal at
            assert len(p) == n
            parts.append(np.asarray(p, dtype=F))
            sets[name] = slice(at, at + n)
            at += n

        cand, a, b, c = candidates(vertices, triangles)
        good = np.nonzero(cand)[0]
        if len(good):
            pick = good[rng.integers(0, len(good), n)]
            a, b = a[pick], b[pick]
        else:
            a = b = np.zeros((n, 3), dtype=F)
        add("uniform", low + rng.uniform(0, 1, (n, 3)) * extent)
        add("vertices", a)
        moved = a.copy()
        which = np.arange(n) % 6
        moved[np.arange(n), which // 2] += np.where(which % 2 == 0, -1, 1) * rng.uniform(0.01, 0.5, n).astype(F)
        add("below_above", moved)
        add("lattice", np.stack([axes[x][rng.integers(0, len(axes[x]), n)] for x in range(3)], axis=1))
        add("midpoints", (a + b) * F(0.5))
        faces, corners = [], []
        for which, (origin, cell, cells) in enumerate(grids):
            m = n // 2 if which == 0 else n - n // 2
            origin, cell = np.asarray(origin, dtype=F), np.asarray(cell, dtype=F)
            plane = np.stack([rng.integers(0, count + 1, m) for count in cells], axis=1)
            on_planes = origin + plane.astype(F) * cell                              # fp32: the planes as the library sees them
            p = (origin + rng.uniform(0, 1, (m, 3)) * (np.asarray(cells) * cell)).astype(F)
            axis = rng.integers(0, 3, m)
            p[np.arange(m), axis] = on_planes[np.arange(m), axis]
            faces.append(p)
            corners.append(on_planes)
        add("faces", np.concatenate(faces))
        add("corners", np.concatenate(corners))
        origin, cell, cells = (np.asarray(x, dtype=np.float64) for x in grids[0])
        p = origin + rng.uniform(0, 1, (n, 3)) * cells * cell
        axis, high = (np.arange(n) % 6) // 2, np.arange(n) % 2
        away = rng.uniform(0.01, 2.0, n) * cell[axis]
        p[np.arange(n), axis] = np.where(high, origin[axis] + cells[axis] * cell[axis] + away, origin[axis] - away)
        add("outside", p)
        p = origin + rng.uniform(0, 1, (n, 3)) * cells * cell
        p[np.arange(n), axis] += np.where(high, 1.0, -1.0) * 2.0 ** 12 * cell[axis]
        add("far", p)
        p = (low + rng.uniform(0, 1, (n, 3)) * extent).astype(F)
        p[np.arange(n), rng.integers(0, 3, n)] = np.array([np.nan, np.inf, -np.inf], dtype=F)[np.arange(n) % 3]
        add("not_finite", p)
        all_p.append(np.concatenate(parts))
    return np.stack(all_p), sets


# ------------------------------------------------------------------------------------------------ the meshes of the tests
MESHES = ("sphere", "torus", "plane", "noise", "equal_to_level", "capped_noise", "simplified_kept", "simplified_removed")
BALANCED = ("sphere", "torus", "capped_noise", "simplified_kept")       # closed: every directed edge has its reverse
OFF_LATTICE = ([-0.7, -0.71, -0.69], [0.11, 0.13, 0.17], [13, 11, 9])
GRIDS = ("one_cell", "k2", "k4", "off_lattice", "column_z", "column_x", "bounding")
NOISE_SHAPE = (9, 17, 33)
_PARTS = {}


def noise_lattice(seed=0, fill=-1.0):
    """``(raw field, capped field, level, axes)`` of the uniform noise lattice: capped = ``close_border`` with ``fill``."""
    from tests import components_reference as cc
    axes = [np.linspace(-1, 1, n).astype(F) for n in NOISE_SHAPE]
    field = np.random.default_rng(3 + seed).uniform(-1, 1, NOISE_SHAPE).astype(F)
    capped = cc.clean(field[None], 0.0, close_border=True, fill=fill)["sigma_out"][0]
    return field, capped, 0.0, axes


def part(kind, seed=0):
    """(single-group mesh dict, lattice axes) of one of MESHES; computed once."""
    from tests import components_reference as cc
    from tests import simplify_reference as sp
    from tests import surface_reference as sr
    if (kind, seed) not in _PARTS:
        if kind in ("sphere", "torus"):
            field, axes = (sr.sphere_field if kind == "sphere" else sr.torus_field)(17)
            level = 0.0
        elif kind == "plane":
            field, axes = sr.plane_field()                       # non-uniform axes; the surface is open at the border
            level = 1.4
        elif kind in ("simplified_kept", "simplified_removed"):
            field, axes = sr.sphere_field(33)
            field = cc.clean(field[None], 0.0, close_border=True)["sigma_out"][0]
            fine = sr.extract_surface(field[None], axes, 0.0)
            _PARTS[(kind, seed)] = (sp.simplify_mesh(fine, *sp.lattice_grid(axes, 2), keep_duplicates=kind == "simplified_kept"), axes)
            return _PARTS[(kind, seed)]
        elif kind == "equal_to_level":                           # a third of the entries on the level: dead and degenerate triangles
            axes = [np.linspace(-1, 1, n).astype(F) for n in NOISE_SHAPE]
            field = np.random.default_rng(3 + seed).integers(-1, 2, NOISE_SHAPE).astype(F) * F(0.5) + F(0.25)
            level = 0.25
        else:
            raw, capped, level, axes = noise_lattice(seed)
            field = raw if kind == "noise" else capped
        _PARTS[(kind, seed)] = (sr.extract_surface(field[None], axes, level), axes)
    return _PARTS[(kind, seed)]


def pack(parts):
    """Packed dict of single-group mesh dicts."""
    return {"vertices": np.concatenate([p["vertices"] for p in parts]).reshape(-1, 3).astype(F),
            "triangles": np.concatenate([p["triangles"] for p in parts]).reshape(-1, 3).astype(np.int32),
            "vertex_offsets": np.concatenate([[0], np.cumsum([len(p["vertices"]) for p in parts])]).astype(np.int32),
            "triangle_offsets": np.concatenate([[0], np.cumsum([len(p["triangles"]) for p in parts])]).astype(np.int32)}


def mesh_case(kind, groups):
    """(packed mesh, axes of the first group's lattice): one group, or three - the mesh, a sphere or torus, the mesh of another seed."""
    first, axes = part(kind)
    if groups == 1:
        parts = [first]
    else:
        parts = [first, part("torus" if kind == "sphere" else "sphere")[0], part(kind, seed=1)[0]]
    return pack(parts), axes


def bounding_grid(mesh, cells):
    """``surface.bounding_grid`` restated: cell = extent / (cells - 1/4), origin = lowest - cell / 8, over the finite vertices."""
    v = mesh["vertices"].astype(np.float64)
    v = v[np.isfinite(v).all(axis=1)]
    origin, cell = [], []
    for a in range(3):
        lowest, highest = float(v[:, a].min()), float(v[:, a].max())
        extent = max(highest - lowest, 2.0 ** -10 * max(1.0, abs(lowest)))
        cell.append(extent / (cells[a] - 0.25))
        origin.append(lowest - cell[a] / 8)
    return origin, cell, list(cells)


def make_grid(name, axes, mesh):
    """One of GRIDS as (origin, cell, cells): one cell; the lattice grid at 2 and 4 steps; the off-lattice grid (part of every mesh is
    loose in it); 1 x 1 x 64 and 64 x 1 x 1; the bounding grid of the mesh."""
    from tests import simplify_reference as sp
    first, extent = [float(a[0]) for a in axes], [float(a[-1]) - float(a[0]) for a in axes]
    if name[0] == "k":
        return sp.lattice_grid(axes, int(name[1:]))
    if name == "one_cell":
        return first, extent, [1, 1, 1]
    if name == "column_z":
        return first, [extent[0], extent[1], extent[2] / 64], [1, 1, 64]
    if name == "column_x":
        return first, [extent[0] / 64, extent[1], extent[2]], [64, 1, 1]
    if name == "bounding":
        return bounding_grid(mesh, (6, 7, 5))
    return OFF_LATTICE


def points_per_set(mesh):
    return 192 if mesh["triangle_offsets"][-1] < 12000 else 48

"""Closest-point queries restated in numpy fp32 as an exhaustive search (not a test).

An independent statement of what ``pr_closest_query`` (include/playrender.h) returns: every point of a group is tested against every
candidate triangle of the group with the header's fp32 formulas in the header's order, and the lexicographic minimum of (dist2,
triangle index) is taken.  There is no grid in ``closest``; the GPU tests check that the grid changes nothing.  ``check_float64`` is a
float64 check of a result for the property tests, ``walk`` restates the kernel's shell walk over the lists of
``raycast_reference.grid_lists`` (it is compared with the search on the CPU, and counts what the walk visits).  Nothing here imports
the package.
"""
import numpy as np

from tests.raycast_reference import F, dot, grid_lists, group_slices

REGIONS = ("vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "interior")


def candidates(vertices, triangles):
    """``(alive (T) bool, a, b, c (T, 3))``: a triangle with an index outside [0, V_g), or a == b or a == c as values, is dead - no
    candidate (the header's rule; the vertices of a dead triangle are returned as those of index 0)."""
    T = len(triangles)
    valid = np.all((triangles >= 0) & (triangles < len(vertices)), axis=1) if len(vertices) else np.zeros(T, dtype=bool)
    if not valid.any():
        z = np.zeros((T, 3), dtype=vertices.dtype)
        return np.zeros(T, dtype=bool), z, z, z
    tri = np.where(valid[:, None], triangles, 0)
    a, b, c = vertices[tri[:, 0]], vertices[tri[:, 1]], vertices[tri[:, 2]]
    with np.errstate(all="ignore"):
        dead = ~valid | np.all(a == b, axis=1) | np.all(a == c, axis=1)
    return ~dead, a, b, c


def _pick(region, options):
    out = options[-1]
    for k in range(len(options) - 2, -1, -1):
        out = np.where(region == k, options[k], out)
    return out


def point_triangle_tests(a, b, c, points):
    """All points (n, 3) against all triangles (a, b, c (T, 3)) in the dtype of the inputs: ``dist2 (n, T)``, ``v``, ``w (n, T)``,
    ``q (n, T, 3)``, ``region (n, T)`` (index into REGIONS).  Ericson's region walk, every operation rounded on its own."""
    dtype = points.dtype
    assert a.dtype == b.dtype == c.dtype == dtype
    one, zero = dtype.type(1), dtype.type(0)
    a, b, c, p = a[None], b[None], c[None], points[:, None, :]
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        ap = p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conditions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                      (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        region = np.full(d1.shape, 6, dtype=np.int8)
        for k in range(5, -1, -1):
            region = np.where(conditions[k], np.int8(k), region)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        v_bc = one - w_bc
        denom = (va + vb) + vc
        v_in, w_in = vb / denom, vc / denom
        v_in = np.where(v_in >= 0, v_in, zero)                           # clamped into the triangle: a NaN or negative quotient is 0,
        v_in = np.where(v_in > one, one, v_in)                           # v at most 1, w at most 1 - v
        w_in = np.where(w_in >= 0, w_in, zero)
        w_in = np.where(w_in > one - v_in, one - v_in, w_in)
        zeros, ones = np.zeros_like(d1), np.ones_like(d1)
        v = _pick(region, [zeros, ones, v_ab, zeros, zeros, v_bc, v_in])
        w = _pick(region, [zeros, zeros, zeros, ones, w_ac, w_bc, w_in])
        r3 = region[..., None]
        shape = ap.shape
        q = _pick(r3, [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + v_ab[..., None] * ab, np.broadcast_to(c, shape),
                       a + w_ac[..., None] * ac, b + w_bc[..., None] * bc, (a + v_in[..., None] * ab) + w_in[..., None] * ac])
        r = p - q
        dist2 = dot(r, r)
    assert dist2.dtype == dtype and v.dtype == dtype and w.dtype == dtype and q.dtype == dtype and zero.dtype == dtype
    return dist2, v, w, q, region


def squared_radius(max_distance):
    with np.errstate(all="ignore"):
        return F(max_distance) * F(max_distance)


def pair_table(mesh, points, pairs=1 << 19):
    """Per group the full table of the exhaustive search: dict(alive (T), dist2, v, w (N, T), q (N, T, 3), region (N, T)) in fp32."""
    points = np.asarray(points, dtype=F)
    out = []
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        alive, a, b, c = candidates(vertices, triangles)
        N, T = points.shape[1], len(triangles)
        table = {"alive": alive, "dist2": np.zeros((N, T), F), "v": np.zeros((N, T), F), "w": np.zeros((N, T), F),
                 "q": np.zeros((N, T, 3), F), "region": np.zeros((N, T), np.int8)}
        rows = max(1, pairs // max(T, 1))
        for r0 in range(0, N if T else 0, rows):
            sl = slice(r0, min(N, r0 + rows))
            table["dist2"][sl], table["v"][sl], table["w"][sl], table["q"][sl], table["region"][sl] = point_triangle_tests(a, b, c, points[g, sl])
        out.append(table)
    return out


def accepted_pairs(table, points_g, max_distance):
    """(N, T) bool: the header's acceptance."""
    with np.errstate(all="ignore"):
        finite = np.isfinite(points_g).all(axis=1)
        return (table["dist2"] <= squared_radius(max_distance)) & (table["dist2"] < F(np.inf)) & table["alive"][None] & finite[:, None]


def closest(mesh, points, max_distance, tables=None):
    """``mesh``: the packed dict of tests/surface_reference.py; ``points (G, N, 3)``.  Returns ``distance (G, N)`` fp32 (+inf: miss),
    ``triangle (G, N)`` int32 (-1), ``point (G, N, 3)`` and ``barycentric (G, N, 2)`` (zeros), and for the property tests ``dist2``
    (+inf), ``accepted (G, N)`` - how many triangles accept the point -, ``ties (G, N)`` - how many of them at the smallest dist2 - and
    ``region (G, N)`` of the winner (-1).  ``tables``: ``pair_table(mesh, points)`` if the caller has it (several radii share one)."""
    points = np.asarray(points, dtype=F)
    G, N = points.shape[:2]
    tables = pair_table(mesh, points) if tables is None else tables
    assert len(tables) == G and points.shape == (G, N, 3)
    out = {"distance": np.full((G, N), np.inf, dtype=F), "triangle": np.full((G, N), -1, dtype=np.int32),
           "point": np.zeros((G, N, 3), dtype=F), "barycentric": np.zeros((G, N, 2), dtype=F), "dist2": np.full((G, N), np.inf, dtype=F),
           "accepted": np.zeros((G, N), dtype=np.int64), "ties": np.zeros((G, N), dtype=np.int64), "region": np.full((G, N), -1, dtype=np.int64)}
    for g, table in enumerate(tables):
        if table["dist2"].shape[1] == 0 or N == 0:
            continue
        accepted = accepted_pairs(table, points[g], max_distance)
        masked = np.where(accepted, table["dist2"], F(np.inf))
        least = masked.min(axis=1)
        at_least = accepted & (table["dist2"] == least[:, None])
        hit = accepted.any(axis=1)
        index = np.argmax(at_least, axis=1)                           # the lowest index among equal dist2
        pick = lambda x: x[np.arange(N), index]
        out["dist2"][g] = np.where(hit, pick(table["dist2"]), F(np.inf))
        out["distance"][g] = np.where(hit, np.sqrt(pick(table["dist2"])), F(np.inf))
        out["triangle"][g] = np.where(hit, index, -1)
        out["point"][g] = np.where(hit[:, None], pick(table["q"]), F(0))
        out["barycentric"][g, :, 0] = np.where(hit, pick(table["v"]), F(0))
        out["barycentric"][g, :, 1] = np.where(hit, pick(table["w"]), F(0))
        out["region"][g] = np.where(hit, pick(table["region"]), -1)
        out["accepted"][g] = accepted.sum(axis=1)
        out["ties"][g] = at_least.sum(axis=1)
    assert out["distance"].dtype == F
    return out


def check_float64(mesh, points, result, max_distance, optimal=True, rows=None):
    """Float64, raises AssertionError: every reported hit is an accepted candidate of the rule - a live triangle of the group,
    barycentrics inside it, ``point`` = a + v (b - a) + w (c - a) and ``distance`` = |p - point| up to fp32 rounding, within
    ``max_distance`` - and (``optimal``) no candidate triangle is closer, in an exact float64 search, than ``distance`` by more than a
    relative 1e-5 plus 1e-6 of the coordinates' scale (a point ON the surface has a distance that is rounding noise), and a miss has no
    candidate within (1 - 1e-5) ``max_distance``.  ``rows``: a slice of the points to check (default: all).  Returns the largest
    deviations, for printing."""
    points = np.asarray(points, dtype=F)
    worst = {"point": 0.0, "distance": 0.0, "closer": 0.0}
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        sl = slice(None) if rows is None else rows
        p = points[g][sl].astype(np.float64)
        tri, dist = result["triangle"][g][sl], result["distance"][g][sl].astype(np.float64)
        hit = tri >= 0
        assert np.all(np.isinf(dist[~hit])) and np.all(np.isfinite(dist[hit]))
        alive, a, b, c = candidates(vertices.astype(np.float64), triangles)
        if hit.any():
            assert tri[hit].max() < len(triangles) and alive[tri[hit]].all()
            assert np.all(dist[hit] <= float(max_distance) * (1 + 1e-6))
            ta, tb, tc = a[tri[hit]], b[tri[hit]], c[tri[hit]]
            scale = np.maximum(1.0, np.max(np.abs(np.stack([ta, tb, tc, p[hit]])), axis=(0, 2)))
            if "barycentric" in result:
                v, w = result["barycentric"][g][sl][hit].astype(np.float64).T
                assert v.min() >= -1e-6 and w.min() >= -1e-6 and (v + w).max() <= 1 + 1e-6
                on_triangle = ta + v[:, None] * (tb - ta) + w[:, None] * (tc - ta)
            if "point" in result:
                q = result["point"][g][sl][hit].astype(np.float64)
                if "barycentric" in result:
                    worst["point"] = max(worst["point"], float((np.linalg.norm(q - on_triangle, axis=1) / scale).max()))
                off = np.abs(np.linalg.norm(p[hit] - q, axis=1) - dist[hit]) / np.maximum(scale, dist[hit])
                worst["distance"] = max(worst["distance"], float(off.max()))
        if optimal and alive.any() and len(p):
            finite = np.isfinite(p).all(axis=1)
            d2 = point_triangle_tests(a[alive], b[alive], c[alive], np.where(finite[:, None], p, 0.0))[0]
            with np.errstate(all="ignore"):
                least = np.sqrt(np.nanmin(np.where(np.isfinite(d2), d2, np.inf), axis=1))
            scale = np.maximum(1.0, np.abs(p).max(axis=1, initial=0.0))
            ok = hit & finite
            closer = (dist[ok] * (1 - 1e-5) - least[ok]) / scale[ok]
            if ok.any():
                worst["closer"] = max(worst["closer"], float(closer.max()))
            missed = ~hit & finite
            assert np.all(least[missed] >= float(max_distance) * (1 - 1e-5) - 1e-6 * scale[missed])
    assert worst["point"] <= 1e-5 and worst["distance"] <= 1e-5 and worst["closer"] <= 1e-6, worst
    return worst


# ------------------------------------------------------------------------------------------------ the kernel's walk restated
def start_cell(point, origin, cell, cells):
    """The header's start cell of a finite point: the cell of (p - origin) / cell in fp32, each index clamped into [0, cells_k)."""
    with np.errstate(all="ignore"):
        g = (np.asarray(point, dtype=F) - np.asarray(origin, dtype=F)) / np.asarray(cell, dtype=F)
    s = []
    for k in range(3):
        x = g[k]
        if not x >= 0:
            x = F(0)
        if x > F(cells[k] - 1):
            x = F(cells[k] - 1)
        s.append(int(x))
    return s


def walk(mesh, origin, cell, cells, points, max_distance, tables=None, lists=None):
    """The shell walk of ``k_closest_query`` over the build's lists, with the arithmetic of the table: the same keys as ``closest``
    (bit-equal inside the header's domain - that is the claim under test), and ``cells_tested`` / ``triangles_tested (G, N)``."""
    points = np.asarray(points, dtype=F)
    G, N = points.shape[:2]
    tables = pair_table(mesh, points) if tables is None else tables
    lists = grid_lists(mesh, origin, cell, cells) if lists is None else lists
    C = int(cells[0]) * int(cells[1]) * int(cells[2])
    cmin = np.asarray(cell, dtype=F).min()
    m2 = squared_radius(max_distance)
    out = {"distance": np.full((G, N), np.inf, dtype=F), "triangle": np.full((G, N), -1, dtype=np.int32),
           "point": np.zeros((G, N, 3), dtype=F), "barycentric": np.zeros((G, N, 2), dtype=F),
           "cells_tested": np.zeros((G, N), dtype=np.int64), "triangles_tested": np.zeros((G, N), dtype=np.int64)}
    for g, table in enumerate(tables):
        accepted = accepted_pairs(table, points[g], max_distance)
        tight = sum(len(l) for l in lists[g][:C])
        for i in range(N):
            if not np.isfinite(points[g, i]).all():
                continue
            best2, best = F(np.inf), -1

            def test(members):
                nonlocal best2, best
                out["triangles_tested"][g, i] += len(members)
                members = members[accepted[i, members]]
                if len(members):
                    d2 = table["dist2"][i, members]
                    k = members[d2 == d2.min()].min()
                    if best < 0 or table["dist2"][i, k] < best2 or (table["dist2"][i, k] == best2 and k < best):
                        best2, best = table["dist2"][i, k], int(k)

            test(lists[g][C])
            if tight:
                s = start_cell(points[g, i], origin, cell, cells)
                last = max(max(s[k], cells[k] - 1 - s[k]) for k in range(3))
                for r in range(last + 1):
                    lo = [max(s[k] - r, 0) for k in range(3)]
                    hi = [min(s[k] + r, cells[k] - 1) for k in range(3)]
                    for x in range(lo[0], hi[0] + 1):
                        for y in range(lo[1], hi[1] + 1):
                            face = max(abs(x - s[0]), abs(y - s[1])) == r
                            for z in (range(lo[2], hi[2] + 1) if face else [z for z in (s[2] - r, s[2] + r) if 0 <= z < cells[2]]):
                                out["cells_tested"][g, i] += 1
                                test(lists[g][(x * cells[1] + y) * cells[2] + z])
                    reach = F(r) * cmin
                    reach2 = reach * reach
                    if (best >= 0 and best2 <= reach2) or reach2 > m2:
                        break
            if best >= 0:
                out["distance"][g, i] = np.sqrt(best2)
                out["triangle"][g, i] = best
                out["point"][g, i] = table["q"][i, best]
                out["barycentric"][g, i] = (table["v"][i, best], table["w"][i, best])
    return out


# ------------------------------------------------------------------------------------------------ point sets the tests share
def triangle_points(vertices, triangles, rng, n):
    """``n`` live, finite triangles drawn at random: (a, b, c (n, 3) fp32, unit normals (n, 3) float64; zero rows if there is none)."""
    alive, a, b, c = candidates(vertices, triangles)
    with np.errstate(all="ignore"):
        normal = np.cross((b - a).astype(np.float64), (c - a).astype(np.float64))
        length = np.linalg.norm(normal, axis=1)
        good = np.nonzero(alive & np.isfinite(length) & (length > 1e-12))[0]
    if len(good) == 0:
        z = np.zeros((n, 3), dtype=F)
        return z, z, z, np.zeros((n, 3))
    k = good[rng.integers(0, len(good), n)]
    return a[k], b[k], c[k], normal[k] / length[k, None]


SETS = ("vertices", "midpoints", "centroids", "quarter", "three", "centre", "faces", "corners", "near_outside", "far", "beyond", "not_finite")


def unit(rng, n):
    x = rng.normal(size=(n, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def point_batch(mesh, axes, n, grids, far_step, seed=0):
    """``(points (G, 12 n, 3), sets)``: the twelve point sets of the tests, ``n`` points each, concatenated; ``sets`` names the slices.
    ``grids``: two (origin, cell, cells) - the sets on cell faces and corners use both, and "a cell" below is the smallest cell size of
    the first.  On mesh vertices (copies), edge midpoints and centroids of random live triangles; centroids moved along the normal by
    a quarter of a cell and by three cells, sides alternating; the lattice's centre (the first point) and points within a hundredth
    of a cell of it; on cell faces and cell corners; up to two cells outside the first grid's box; 1 000 ``far_step`` away (the
    smallest cell size of all grids the batch is used with: inside the domain of the guarantee on each); 2^13 to 2^14 cells away
    (beyond the domain); a NaN or an infinite component."""
    rng = np.random.default_rng(200 + seed)
    centre = np.array([(float(a[0]) + float(a[-1])) / 2 for a in axes])
    step = float(np.min(np.asarray(grids[0][1], dtype=np.float64)))
    all_p, sets = [], {}
    for g, (vertices, triangles) in enumerate(group_slices(mesh)):
        parts, at = [], 0

        def add(name, p):
            nonlocal at
            assert len(p) == n
            parts.append(np.asarray(p, dtype=F))
            sets[name] = slice(at, at + n)
            at += n

        a, b, c, normal = triangle_points(vertices, triangles, rng, n)
        add("vertices", a)
        add("midpoints", (a + b) * F(0.5))
        centroid = ((a + b) + c) / F(3)
        add("centroids", centroid)
        side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
        add("quarter", centroid + side * 0.25 * step * normal)
        add("three", centroid + side * 3.0 * step * normal)
        near = centre + 0.01 * step * unit(rng, n)
        near[0] = centre
        add("centre", near)
        faces, corners = [], []
        for k, (origin, cell, cells) in enumerate(grids):
            m = n // 2 if k == 0 else n - n // 2
            origin, cell = np.asarray(origin, dtype=F), np.asarray(cell, dtype=F)
            plane = np.stack([rng.integers(0, c + 1, m) for c in cells], axis=1)
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
        axis, high = rng.integers(0, 3, n), rng.integers(0, 2, n)
        away = rng.uniform(0.01, 2.0, n) * cell[axis]
        p[np.arange(n), axis] = np.where(high, origin[axis] + cells[axis] * cell[axis] + away, origin[axis] - away)
        add("near_outside", p)
        add("far", centre + 1000.0 * float(far_step) * unit(rng, n))
        add("beyond", centre + rng.uniform(2.0 ** 13, 2.0 ** 14, (n, 1)) * step * unit(rng, n))
        p = (centre + step * unit(rng, n)).astype(F)
        p[np.arange(n), rng.integers(0, 3, n)] = np.array([np.nan, np.inf, -np.inf], dtype=F)[np.arange(n) % 3]
        add("not_finite", p)
        all_p.append(np.concatenate(parts))
    return np.stack(all_p), sets

"""Mesh intersection restated in numpy fp32 as an exhaustive rule (not a test).

An independent statement of what ``pr_mesh_intersect`` (include/playrender.h) returns: every query triangle of a group is tested
against every target triangle of the group with the header's fp32 formulas in the header's order - BOX, the six edge tests of
``raycast_reference.ray_triangle_tests`` with ``t`` in [0, 1], the conditioning clause - and the pairs, their counts and their contact
segments are collected.  There is no grid here - the GPU tests check that the grid changes nothing.  ``plane_distance`` is a float64
check of the segment endpoints for the property tests.  Nothing here imports the package.
"""
import numpy as np

from tests.raycast_reference import F, SLIVER, cross, dot, group_slices, clamped_offsets, ray_triangle_tests

EDGES = ((0, 1), (1, 2), (2, 0))


def transformed(vertices, m):
    """``x'_k = ((m_k0 x_0 + m_k1 x_1) + m_k2 x_2) + m_k3`` in fp32; ``m (3, 4)`` or None."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    if m is None:
        return v
    m = np.asarray(m, dtype=F)
    with np.errstate(all="ignore"):
        return np.stack([((m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2]) + m[k, 3] for k in range(3)], axis=1)


def corners(vertices, triangles):
    """``(corner rows (T, 3, 3), candidate (T))``: three indices in range and nine finite coordinates."""
    T = len(triangles)
    if len(vertices) == 0 or T == 0:
        return np.zeros((T, 3, 3), dtype=F), np.zeros(T, dtype=bool)
    valid = np.all((triangles >= 0) & (triangles < len(vertices)), axis=1)
    x = vertices[np.where(valid[:, None], triangles, 0)]
    return x, valid & np.isfinite(x).all(axis=(1, 2))


def _edge_rays(x):
    """The three edges of every triangle as rays: ``(origins, directions) (n, 3 edges, 3)``."""
    with np.errstate(all="ignore"):
        return np.stack([x[:, i] for i, _ in EDGES], axis=1), np.stack([x[:, j] - x[:, i] for i, j in EDGES], axis=1)


def _accepted(o, d, vertices, triangles, condition):
    """Rays ``(n, 3)`` against the triangles: ``accepted (n, T)`` of the header's test with t in [0, 1] and the clause, and ``t``."""
    accepted, t, _, _, det = ray_triangle_tests(vertices, triangles, o, d, 0.0, 1.0, False)
    if condition and accepted.any():
        x, _ = corners(vertices, triangles)
        with np.errstate(all="ignore"):
            e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
            ee = dot(e1, e1) * dot(e2, e2)
            accepted = accepted & (det * det > SLIVER * (ee[None, :] * dot(d, d)[:, None]))
    return accepted, t


def group_pairs(tv, tt, qv, qt, self_=False, box=True, condition=True, budget=1 << 21):
    """One group: target vertices / triangles, query vertices (already transformed) / triangles.  Returns ``pairs (P, 2)`` sorted by
    (query, target), ``segments (P, 2, 3)``, ``accepted (P)`` - the accepted edge tests of every pair, 1 .. 6 - and the number of
    candidate pairs that the edge tests accept although BOX fails (they are pairs only with ``box=False``)."""
    tx, tcand = corners(tv, tt)
    qx, qcand = corners(qv, qt)
    with np.errstate(all="ignore"):
        tcand = tcand & ~np.all(tx[:, 0] == tx[:, 1], axis=1) & ~np.all(tx[:, 0] == tx[:, 2], axis=1)        # dead targets
    pairs, segments, counts, outside = [], [], [], 0
    T, QT = len(tt), len(qt)
    if T == 0 or QT == 0 or not tcand.any() or not qcand.any():
        return np.zeros((0, 2), np.int32), np.zeros((0, 2, 3), F), np.zeros(0, np.int64), 0
    to, td = _edge_rays(tx)
    tlo, thi = tx.min(axis=1), tx.max(axis=1)
    rows = max(1, budget // (3 * T))
    for r0 in range(0, QT, rows):
        sl = slice(r0, min(QT, r0 + rows))
        n = sl.stop - sl.start
        qo, qd = _edge_rays(qx[sl])
        acc = np.zeros((n, T, 6), dtype=bool)
        t = np.zeros((n, T, 6), dtype=F)
        a, tq = _accepted(qo.reshape(-1, 3), qd.reshape(-1, 3), tv, tt, condition)                          # (3 n, T)
        acc[:, :, :3], t[:, :, :3] = a.reshape(n, 3, T).transpose(0, 2, 1), tq.reshape(n, 3, T).transpose(0, 2, 1)
        a, tq = _accepted(to.reshape(-1, 3), td.reshape(-1, 3), qv, qt[sl], condition)                      # (3 T, n)
        acc[:, :, 3:], t[:, :, 3:] = a.reshape(T, 3, n).transpose(2, 0, 1), tq.reshape(T, 3, n).transpose(2, 0, 1)
        allowed = qcand[sl, None] & tcand[None, :]
        if self_:
            allowed &= np.arange(sl.start, sl.stop)[:, None] != np.arange(T)[None, :]
            with np.errstate(all="ignore"):
                shared = np.zeros((n, T), dtype=bool)
                for i in range(3):
                    for j in range(3):
                        shared |= np.all(qx[sl, None, i] == tx[None, :, j], axis=-1)
            allowed &= ~shared
        qlo, qhi = qx[sl].min(axis=1), qx[sl].max(axis=1)
        with np.errstate(all="ignore"):
            inbox = np.all((qlo[:, None] <= thi[None]) & (tlo[None] <= qhi[:, None]), axis=-1)
        edge = acc.any(axis=-1) & allowed
        outside += int((edge & ~inbox).sum())
        found = edge & inbox if box else edge
        qi, ti = np.nonzero(found)                                         # (row-major: sorted by query, then target)
        if len(qi) == 0:
            continue
        a6, t6 = acc[qi, ti], t[qi, ti]                                    # (P, 6)
        o6 = np.concatenate([qo[qi], to[ti]], axis=1)                      # (P, 6, 3): Q's three edges, then T's
        d6 = np.concatenate([qd[qi], td[ti]], axis=1)
        with np.errstate(all="ignore"):
            points = o6 + t6[:, :, None] * d6
        P = len(qi)
        p0, p1, far, seen = np.zeros((P, 3), F), np.zeros((P, 3), F), np.zeros(P, F), np.zeros(P, np.int64)
        for k in range(6):
            start = a6[:, k] & (seen == 0)
            p0[start] = p1[start] = points[start, k]
            with np.errstate(all="ignore"):
                r = points[:, k] - p0
                d2 = dot(r, r)
            better = a6[:, k] & (seen > 0) & (d2 > far)
            far[better], p1[better] = d2[better], points[better, k]
            seen += a6[:, k]
        pairs.append(np.stack([qi + sl.start, ti], axis=1).astype(np.int32))
        segments.append(np.stack([p0, p1], axis=1))
        counts.append(seen)
    if not pairs:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2, 3), F), np.zeros(0, np.int64), outside
    return np.concatenate(pairs), np.concatenate(segments), np.concatenate(counts), outside


def intersect(target, query=None, transform=None, self_=False, box=True, condition=True):
    """``target`` / ``query``: packed dicts of tests/surface_reference.py (``V`` / ``T``: the totals the call is told, default: the
    rows); ``transform (G, 3, 4)`` or None; ``self_``: the target against itself.  Returns ``count (QT)``, ``first (QT)``,
    ``pair_offsets (QT + 1)`` in the packed order of the query triangles, ``pairs (P, 2)`` local to their group and sorted by (packed
    query row, target), ``rows (P)`` - the packed query row of every pair -, ``groups (P)``, ``segments (P, 2, 3)``, ``accepted (P)``
    and ``outside_box`` (see ``group_pairs``)."""
    query = target if self_ else query
    tg, qg = group_slices(target), group_slices(query)
    assert len(tg) == len(qg)
    QT = int(query.get("T", len(np.asarray(query["triangles"]).reshape(-1, 3))))
    first_row = clamped_offsets(query["triangle_offsets"], QT)
    count, first = np.zeros(QT, dtype=np.int32), np.full(QT, -1, dtype=np.int32)
    pairs, rows, groups, segments, accepted, outside = [], [], [], [], [], 0
    for g, ((tv, tt), (qv, qt)) in enumerate(zip(tg, qg)):
        m = None if transform is None else np.asarray(transform, dtype=F)[g]
        p, s, a, o = group_pairs(tv, tt, transformed(qv, m), qt, self_, box, condition)
        outside += o
        if len(p):
            own = count[first_row[g]:first_row[g + 1]]
            own += np.bincount(p[:, 0], minlength=len(own)).astype(np.int32)
            lowest = first[first_row[g]:first_row[g + 1]]
            head = np.concatenate([[True], p[1:, 0] != p[:-1, 0]])       # (sorted: the first row of a query has its lowest target)
            lowest[p[head, 0]] = p[head, 1]
        pairs.append(p)
        rows.append(p[:, 0].astype(np.int64) + first_row[g])
        groups.append(np.full(len(p), g, dtype=np.int64))
        segments.append(s)
        accepted.append(a)
    return {"count": count, "first": first, "pair_offsets": np.concatenate([[0], np.cumsum(count)]).astype(np.int32),
            "pairs": np.concatenate(pairs), "rows": np.concatenate(rows), "groups": np.concatenate(groups),
            "segments": np.concatenate(segments), "accepted": np.concatenate(accepted), "outside_box": outside}


def plane_distance(target, query, result, transform=None):
    """Float64: per pair and endpoint the distance of the endpoint from the planes of the query triangle and of the target triangle
    ``(P, 2 endpoints, 2 planes)`` - an independent check that a contact segment lies in both triangles' planes."""
    tg, qg = group_slices(target), group_slices(query)
    out = np.zeros((len(result["pairs"]), 2, 2))
    for g, ((tv, tt), (qv, qt)) in enumerate(zip(tg, qg)):
        at = np.nonzero(result["groups"] == g)[0]
        if len(at) == 0:
            continue
        m = None if transform is None else np.asarray(transform, dtype=F)[g]
        qv = transformed(qv, m)
        for side, (v, tri) in enumerate(((qv, qt[result["pairs"][at, 0]]), (tv, tt[result["pairs"][at, 1]]))):
            a, b, c = (v[tri[:, k]].astype(np.float64) for k in range(3))
            n = np.cross(b - a, c - a)
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            for end in range(2):
                out[at, end, side] = np.abs(np.sum((result["segments"][at, end].astype(np.float64) - a) * n, axis=1))
    return out


def contact_length(result):
    """The float64 sum of the segment lengths."""
    s = result["segments"].astype(np.float64)
    return float(np.linalg.norm(s[:, 1] - s[:, 0], axis=1).sum())


def shifted(mesh, shift):
    """A copy of a packed mesh with every vertex moved by ``shift`` in fp32."""
    out = packed(mesh)
    out["vertices"] = (out["vertices"] + np.asarray(shift, dtype=F)).astype(F)
    return out


def packed(mesh):
    """The four packed arrays of a mesh dict of tests/surface_reference.py (offsets of one group where it has none)."""
    v = np.ascontiguousarray(mesh["vertices"], dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(mesh["triangles"], dtype=np.int32).reshape(-1, 3)
    return {"vertices": v, "triangles": t, "vertex_offsets": np.asarray(mesh.get("vertex_offsets", [0, len(v)]), dtype=np.int32),
            "triangle_offsets": np.asarray(mesh.get("triangle_offsets", [0, len(t)]), dtype=np.int32)}


def joined(a, b):
    """Two single-group meshes as ONE group (the second one's indices moved behind the first one's vertices)."""
    a, b = packed(a), packed(b)
    v = np.concatenate([a["vertices"], b["vertices"]])
    t = np.concatenate([a["triangles"], b["triangles"] + np.int32(len(a["vertices"]))])
    return {"vertices": v, "triangles": t, "vertex_offsets": np.array([0, len(v)], dtype=np.int32),
            "triangle_offsets": np.array([0, len(t)], dtype=np.int32)}

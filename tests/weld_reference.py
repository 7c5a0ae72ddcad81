"""Welding and compaction restated in numpy (not a test).

An independent statement of what ``pr_mesh_weld`` (include/playrender.h) returns, written from the header's words and without a hash
table: the classes and the kept triangles are ``audit_reference.representatives`` / ``candidate_mask``, the output indices a ``cumsum``
over the referenced flags.  Nothing here imports the package.
"""
import numpy as np

from tests import audit_reference as ar
from tests.raycast_reference import clamped_offsets, group_slices

F = np.float32
COUNTS = 8


def weld_group(vertices, triangles, merge=True):
    """One group: a dict with ``keep`` (V_g) bool - the referenced representatives, in output order -, ``triangles`` (kept, 3) int32
    re-indexed, ``vertex_map`` (V_g), ``triangle_map`` (T_g) int32 and ``counts`` (8) int64."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    by_value = ar.representatives(v)
    kept = ar.candidate_mask(v, t, by_value)                        # (by VALUE in both modes)
    rep = by_value if merge else np.where(by_value >= 0, np.arange(V), -1)
    referenced = np.zeros(V, dtype=bool)
    corners = rep[t[kept]] if kept.any() else np.zeros((0, 3), dtype=np.int64)
    referenced[corners.reshape(-1)] = True
    index = np.cumsum(referenced) - 1                               # output index of a referenced representative
    safe = np.maximum(rep, 0)
    vertex_map = np.where((rep >= 0) & referenced[safe], index[safe], -1).astype(np.int32) if V else np.zeros(0, dtype=np.int32)
    triangle_map = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)
    own = np.arange(V)
    counts = np.zeros(COUNTS, dtype=np.int64)
    counts[0], counts[1], counts[2] = int(referenced.sum()), int(kept.sum()), int(T - kept.sum())
    counts[3] = int((rep < 0).sum())
    counts[4] = int(((rep >= 0) & (rep != own)).sum())
    counts[5] = int(((rep == own) & ~referenced).sum())
    return {"keep": referenced, "triangles": index[corners].astype(np.int32).reshape(-1, 3), "vertex_map": vertex_map,
            "triangle_map": triangle_map, "counts": counts}


def weld(mesh, merge=True, normals=None, attributes=None):
    """``mesh``: the packed dict of tests/surface_reference.py (optionally with the totals ``V`` / ``T``); ``normals (V, 3)`` /
    ``attributes (V, A)`` optional arrays whose rows are carried bit for bit.  Returns a dict: ``vertices``, ``triangles``,
    ``vertex_offsets``, ``triangle_offsets`` - a packed mesh again -, ``normals`` / ``attributes`` or None, ``vertex_map (V)``,
    ``triangle_map (T)`` int32 (-1 also for the rows that no clamped group owns) and ``counts (G, 8)`` int32."""
    v = np.ascontiguousarray(mesh["vertices"], dtype=F).reshape(-1, 3)
    t = np.asarray(mesh["triangles"]).reshape(-1, 3)
    V, T = int(mesh.get("V", len(v))), int(mesh.get("T", len(t)))
    vo, to = clamped_offsets(mesh["vertex_offsets"], V), clamped_offsets(mesh["triangle_offsets"], T)
    parts = [weld_group(vertices, triangles, merge) for vertices, triangles in group_slices(mesh)]
    rows = np.concatenate([vo[g] + np.nonzero(p["keep"])[0] for g, p in enumerate(parts)]).astype(np.int64)
    vertex_map, triangle_map = np.full(V, -1, dtype=np.int32), np.full(T, -1, dtype=np.int32)
    for g, p in enumerate(parts):
        vertex_map[vo[g]:vo[g + 1]] = p["vertex_map"]
        triangle_map[to[g]:to[g + 1]] = p["triangle_map"]
    counts = np.stack([p["counts"] for p in parts]).astype(np.int32)
    carried = lambda x: None if x is None else np.ascontiguousarray(x, dtype=F).reshape(V, np.shape(x)[-1]).view(np.uint32)[rows].view(F)
    return {"vertices": v.view(np.uint32)[rows].view(F), "triangles": np.concatenate([p["triangles"] for p in parts]).reshape(-1, 3),
            "vertex_offsets": np.concatenate([[0], np.cumsum(counts[:, 0])]).astype(np.int32),
            "triangle_offsets": np.concatenate([[0], np.cumsum(counts[:, 1])]).astype(np.int32),
            "normals": carried(normals), "attributes": carried(attributes), "vertex_map": vertex_map, "triangle_map": triangle_map,
            "counts": counts}

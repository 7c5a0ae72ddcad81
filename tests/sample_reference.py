"""Area-weighted surface samples restated in numpy and Python integers (not a test).

An independent statement of what ``pr_mesh_sample`` (include/playrender.h) returns, written from the header's words: the areas in numpy
float64 (numpy rounds every operation on its own: no contraction), the weights, their prefix sums, the pick and the barycentric
integers in Python integers, the interpolation in ``np.float32``; Philox4x32-10 and the splitmix64 finaliser are written out.  Nothing
here imports the package, and nothing but numpy and the standard library is used.
"""
import bisect
import itertools

import numpy as np

F = np.float32
COUNTS = 4
MEASURES = 2
FACE_NORMALS = 1
ONE = 1 << 24
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


def noise_mix(x):
    """The splitmix64 finaliser (the key mix of the renderer's noise streams), on a Python integer."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") on arrays (or scalars) of counters held in uint64
    with values below 2^32; the key is a pair of Python integers.  Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)).copy() for c in np.broadcast_arrays(c0, c1, c2, c3))
    mask = np.uint64(M32)
    shift = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                              # (below 2^64: no wrap)
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> shift) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> shift) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & mask, n2, p0 & mask
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def clamped_offsets(offsets, total):
    """Offsets that leave [0, total] or decrease are clamped (the header's rule)."""
    out, at = [], 0
    for x in np.asarray(offsets).tolist():
        at = min(int(total), max(at, int(x)))
        out.append(at)
    return out


def valid_triangles(vertices, triangles):
    """One group: the (T) mask of the valid triangles - three indices in range, pairwise different as indices, nine finite coordinates."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    valid = np.zeros(T, dtype=bool)
    if V and T:
        valid = np.all((t >= 0) & (t < V), axis=1)
        valid &= (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
        safe = np.where(valid[:, None], t, 0)
        valid &= np.isfinite(v[safe].reshape(T, 9)).all(axis=1)
    return valid


def areas(vertices, triangles, valid):
    """The float64 areas of the valid triangles (0 for the others), the audit's expression."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(t))
    rows = np.nonzero(valid)[0]
    if len(rows):
        a, b, c = (v[t[rows, k]].astype(np.float64) for k in range(3))
        e1, e2 = b - a, c - a
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        out[rows] = 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    return out


def group_weights(vertices, triangles):
    """One group: ``(valid (T) bool, area (T) float64, A_max, w (list of T Python integers), W (list: the inclusive prefix sums))``."""
    valid = valid_triangles(vertices, triangles)
    area = areas(vertices, triangles, valid)
    largest = float(area.max()) if len(area) else 0.0
    if largest > 0.0:
        scaled = (area / largest) * 4294967296.0                     # the quotient is rounded, the scaling is exact
        w = [int(x) if ok else 0 for x, ok in zip(scaled.tolist(), valid.tolist())]         # int(): floor of a non-negative value
    else:
        w = [0] * len(area)
    return valid, area, largest, w, list(itertools.accumulate(w))


def draws(n, seed, first, group):
    """The n draws of a group: ``(r (list of Python integers), U, V (int64 arrays, folded))``."""
    key = noise_mix(int(seed) & M64)
    j = [(int(first) + i) & M64 for i in range(n)]
    low = np.array([x & M32 for x in j], dtype=np.uint64)
    high = np.array([x >> 32 for x in j], dtype=np.uint64)
    x0, x1, x2, x3 = philox4x32_10(low, high, np.uint64(group), np.uint64(0), key & M32, key >> 32) if n else (np.zeros(0, np.uint64),) * 4
    r = [int(a) | (int(b) << 32) for a, b in zip(x0.tolist(), x1.tolist())]
    U, V = (x2 >> np.uint64(8)).astype(np.int64), (x3 >> np.uint64(8)).astype(np.int64)
    fold = U + V > ONE
    U, V = np.where(fold, ONE - U, U), np.where(fold, ONE - V, V)
    return r, U, V


def mix(b0, b1, b2, a, b, c):
    """The point formula on float32 arrays: ``((b0 a) + (b1 b)) + (b2 c)``, every operation rounded on its own."""
    b0, b1, b2 = (np.asarray(x, dtype=F)[:, None] for x in (b0, b1, b2))
    with np.errstate(all="ignore"):
        return ((b0 * a.astype(F)) + (b1 * b.astype(F))) + (b2 * c.astype(F))


def normalise(N):
    """``N / sqrt((N0 N0 + N1 N1) + N2 N2)`` in float32 where the length is finite and > 0, else zeros."""
    N = np.asarray(N, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        fine = np.isfinite(length) & (length > 0)
        return np.where(fine[:, None], N / np.where(fine, length, F(1))[:, None], F(0)).astype(F)


def sample_group(vertices, triangles, n, seed, first, group, normals=None, attributes=None, face=False):
    """One group: a dict of ``points (n, 3)``, ``triangle (n)`` int32, ``barycentric (n, 2)``, ``normals (n, 3)`` or None, ``attributes
    (n, C)`` or None, ``counts (4)``, ``measures (2)`` and, for the tests, ``w`` and ``area``."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    valid, area, largest, w, W = group_weights(v, t)
    total = W[-1] if W else 0
    empty = total == 0
    zero_weight = sum(1 for x, ok in zip(w, valid.tolist()) if ok and x == 0)
    out = {"points": np.zeros((n, 3), F), "triangle": np.full(n, -1, np.int32), "barycentric": np.zeros((n, 2), F),
           "normals": np.zeros((n, 3), F) if (face or normals is not None) else None,
           "attributes": None if attributes is None else np.zeros((n, np.asarray(attributes).shape[1]), F),
           "counts": np.array([int(valid.sum()), len(t) - int(valid.sum()), zero_weight, 0 if empty else n], dtype=np.int32),
           "measures": np.array([0.0 if empty else largest, 0.0 if empty else (float(total) * largest) * 2.0 ** -32]),
           "w": w, "area": area, "U": np.zeros(n, np.int64), "V": np.zeros(n, np.int64)}
    if empty or n == 0:
        return out
    r, U, V = draws(n, seed, first, group)
    picked = np.array([bisect.bisect_right(W, (x * total) >> 64) for x in r], dtype=np.int64)     # the first triangle with W_t > pick
    b1, b2, b0 = U.astype(F) * F(2.0 ** -24), V.astype(F) * F(2.0 ** -24), (ONE - U - V).astype(F) * F(2.0 ** -24)
    corners = t[picked]
    a, b, c = (v[corners[:, k]] for k in range(3))
    out["points"] = mix(b0, b1, b2, a, b, c)
    out["triangle"] = picked.astype(np.int32)
    out["barycentric"] = np.stack([b1, b2], axis=1)
    out["U"], out["V"] = U, V
    if face:
        with np.errstate(all="ignore"):
            e1, e2 = b - a, c - a
            N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        out["normals"] = normalise(N)
    elif normals is not None:
        rows = np.asarray(normals, dtype=F).reshape(-1, 3)
        out["normals"] = normalise(mix(b0, b1, b2, *(rows[corners[:, k]] for k in range(3))))
    if attributes is not None:
        rows = np.asarray(attributes, dtype=F)
        out["attributes"] = mix(b0, b1, b2, *(rows[corners[:, k]] for k in range(3)))
    return out


def sample(mesh, n, seed, first=0, normals=None, attributes=None, face=False):
    """``mesh``: the packed dict of tests/surface_reference.py (optionally with the totals ``V`` / ``T``); ``normals (V, 3)`` /
    ``attributes (V, C)`` are packed alongside.  Returns a dict of the header's outputs stacked over the groups - ``points (G, n, 3)``,
    ``triangle (G, n)``, ``barycentric (G, n, 2)``, ``normals``, ``attributes`` (None where not asked for), ``counts (G, 4)`` int32,
    ``measures (G, 2)`` float64 - and ``groups``: the per-group dicts."""
    v = np.asarray(mesh["vertices"], dtype=F).reshape(-1, 3)
    t = np.asarray(mesh["triangles"]).reshape(-1, 3)
    V, T = int(mesh.get("V", len(v))), int(mesh.get("T", len(t)))
    vo, to = clamped_offsets(mesh["vertex_offsets"], V), clamped_offsets(mesh["triangle_offsets"], T)
    parts = []
    for g in range(len(vo) - 1):
        rows = slice(vo[g], vo[g + 1])
        parts.append(sample_group(v[rows], t[to[g]:to[g + 1]], n, seed, first, g, None if normals is None else np.asarray(normals)[rows],
                                  None if attributes is None else np.asarray(attributes)[rows], face))
    out = {"groups": parts}
    for key in ("points", "triangle", "barycentric", "normals", "attributes", "counts", "measures"):
        out[key] = None if parts[0][key] is None else np.stack([p[key] for p in parts])
    return out

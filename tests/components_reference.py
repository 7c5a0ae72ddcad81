"""Numpy restatement of ``pr_label_components`` (include/playrender.h) - not a test: what tests/test_components_*.py compare
against.  Written from the header's contract, with none of the kernel's machinery: labels by propagating the minimum label over the
seven edge directions (both ways) until nothing changes, sizes by counting, the selection rule by sorting."""
import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
CLOSE_BORDER = 1


def inside_mask(sigma, level, close_border=False):
    """``sigma (G, nx, ny, nz)`` -> bool: ``sigma > level`` (never for a NaN), without the border layer when ``close_border``."""
    sigma = np.asarray(sigma, dtype=np.float32)
    assert sigma.ndim == 4
    with np.errstate(invalid="ignore"):
        inside = sigma > np.float32(level)
    if close_border:
        for axis in (1, 2, 3):
            index = [slice(None)] * 4
            for end in (0, sigma.shape[axis] - 1):
                index[axis] = end
                inside[tuple(index)] = False
    return inside


def _label_group(inside):
    shape = inside.shape
    big = np.int64(inside.size)
    label = np.where(inside, np.arange(inside.size, dtype=np.int64).reshape(shape), big)
    while True:
        new = label.copy()
        for d in DIRECTIONS:
            lo = tuple(slice(0, n - s) for n, s in zip(shape, d))      # points p with p + d on the lattice
            hi = tuple(slice(s, n) for n, s in zip(shape, d))          # ... and those p + d
            both = inside[lo] & inside[hi]
            new[lo] = np.where(both, np.minimum(new[lo], label[hi]), new[lo])
            new[hi] = np.where(both, np.minimum(new[hi], label[lo]), new[hi])
        if np.array_equal(new, label):
            break
        label = new
    return np.where(inside, label, -1).astype(np.int32)


def label_components(sigma, level, close_border=False):
    """``(labels, sizes)``, both int32 ``(G, nx, ny, nz)``: the smallest flat index of the point's component (-1 outside) and the
    number of points of that component (0 outside)."""
    inside = inside_mask(sigma, level, close_border)
    labels = np.stack([_label_group(m) for m in inside])
    sizes = np.zeros(labels.shape, dtype=np.int32)
    for g in range(labels.shape[0]):
        roots, counts = np.unique(labels[g][labels[g] >= 0], return_counts=True)
        table = np.zeros(labels[g].size + 1, dtype=np.int32)
        table[roots] = counts
        sizes[g] = np.where(labels[g] >= 0, table[labels[g]], 0)
    return labels, sizes


def components_of(labels, sizes):
    """Per group the list of ``(label, size)``, ranked: size descending, ties by label ascending."""
    out = []
    for g in range(labels.shape[0]):
        roots = np.unique(labels[g][labels[g] >= 0])
        flat = sizes[g].reshape(-1)
        out.append(sorted(((int(r), int(flat[r])) for r in roots), key=lambda c: (-c[1], c[0])))
    return out


def kept_labels(ranked, min_points=0, keep_largest=0):
    """The labels of one group's kept components: ``size >= min_points`` and (``keep_largest == 0`` or ``rank < keep_largest``)."""
    return [label for rank, (label, size) in enumerate(ranked) if size >= min_points and (keep_largest == 0 or rank < keep_largest)]


def clean(sigma, level, min_points=0, keep_largest=0, close_border=False, fill=None):
    """The full call: a dict of ``labels``, ``sizes`` (int32), ``sigma_out`` (fp32: ``fill`` - default ``level`` - at the inside points
    of components that are not kept and, with ``close_border``, at border points ``> level``; the input bits elsewhere) and ``counts
    (G, 4)`` int32 = inside points, components, kept components, kept points."""
    sigma = np.ascontiguousarray(sigma, dtype=np.float32)
    fill = np.float32(level if fill is None else fill)
    assert fill <= np.float32(level)
    labels, sizes = label_components(sigma, level, close_border)
    ranked = components_of(labels, sizes)
    out = sigma.copy()
    counts = np.zeros((sigma.shape[0], 4), dtype=np.int32)
    for g in range(sigma.shape[0]):
        kept = kept_labels(ranked[g], min_points, keep_largest)
        keep_point = np.isin(labels[g], kept) & (labels[g] >= 0)
        out[g][(labels[g] >= 0) & ~keep_point] = fill
        counts[g] = [int((labels[g] >= 0).sum()), len(ranked[g]), len(kept), int(keep_point.sum())]
    if close_border:
        out[inside_mask(sigma, level, False) & ~inside_mask(sigma, level, True)] = fill          # border points > level
    return {"labels": labels, "sizes": sizes, "sigma_out": out, "counts": counts}


def bits(a):
    """fp32 values as their int32 bit patterns (so that NaNs compare)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the fields the tests share
def two_blob_field(n):
    """Two balls on ``x = linspace(-1, 1, n)`` (level 0) and five isolated 1.0s: two single points, a pair along (-1, 1, 1) - not an
    edge direction, so two more singles - and a pair along (1, 1, 1) that touches the border.  Returns (field, axes)."""
    x = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    f = np.maximum(0.25 - (X + 0.3) ** 2 - Y ** 2 - Z ** 2, 0.04 - (X - 0.7) ** 2 - (Y - 0.6) ** 2 - (Z - 0.6) ** 2).astype(np.float32)
    for at in ((1, 1, 1), (n - 2, 1, 2), (n - 3, 2, 3), (1, n - 2, 1), (2, n - 1, 2)):
        f[at] = 1.0
    return f, [x.astype(np.float32)] * 3

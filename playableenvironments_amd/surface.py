"""Triangle meshes of density lattices (``pr_extract_surface``, include/playrender.h): marching tetrahedra on the Freudenthal
(Kuhn) split, on the device - what ``ObjectComposer.extract_mesh`` turns the output of ``density_grid`` into.

``extract_surface`` takes a lattice ``sigma (G, nx, ny, nz)`` with the three coordinate vectors of its points and a raw-density
``level`` and returns one ``Mesh`` per group: indexed, closed inside the lattice (a surface that reaches the lattice border is open
there), triangle normals pointing from matter (``sigma > level``) to empty space.  Lattice values exactly equal to ``level`` count
as outside and give coinciding vertices and zero-area triangles, which are kept.  The vertex and triangle order is fixed (header),
so results can be compared bit for bit.  There is no CPU fallback.

``label_components`` / ``clean_lattice`` (``pr_label_components``) label the connected components of the inside set on the same
lattice and blank out the unwanted ones: floater removal (``keep_largest``, ``min_points``) and capping (``close_border``) in front of
the mesher and of ``pr_occupancy_build``.

``refine_band`` (``pr_band_plan`` / ``pr_band_fill``) fills a lattice from its coarse skeleton and evaluates the field only in a band
around the level set - the opt-in approximation behind ``ObjectComposer.density_band`` and ``extract_mesh(stride=...)``.

``simplify_meshes`` / ``Mesh.simplified`` (``pr_simplify_mesh``) reduce extracted meshes by vertex clustering on a uniform grid, on
the device and independent of the execution order - what ``extract_surface(simplify=k)`` and ``extract_mesh(simplify=k)`` apply.
``placement="quadric"`` / ``place_vertices`` (``pr_mesh_place``) then move every cluster's vertex from the mean of its members to the
point that the planes of its triangles ask for: edges and corners stay sharp, and most of the volume that the mean loses is kept.

``RayGrid`` / ``Mesh.ray_grid`` (``pr_raycast_build`` / ``pr_raycast_query``) answer closest-hit ray queries against such meshes on a
uniform cell grid: ``RayGrid.build(meshes, *bounding_grid(meshes, 32)).cast(origins, directions)``.  ``RayGrid.closest``
(``pr_closest_query``) finds the closest point of a mesh to a point on the same grid, and ``Mesh.distance_to`` measures how far one mesh
lies from another with it.  ``RayGrid.winding`` / ``contains`` / ``signed_distance`` (``pr_inside_query``) decide on the same grid whether
a point lies inside a mesh - watertight by construction, for capped meshes (``close_border=True``) that kept their duplicates when
simplified (``keep_duplicates=True``).

``audit_meshes`` / ``Mesh.audit`` / ``RayGrid.audit`` (``pr_mesh_audit``) say how a mesh is made up - whether its directed edges balance
by vertex value (what ``contains`` needs), boundary and non-manifold edges, Euler characteristic, shells, area, signed volume, centroid -
and ``Mesh.keep_shells`` drops the fragments that a simplification detached.

``weld_meshes`` / ``Mesh.welded`` / ``Mesh.compacted`` (``pr_mesh_weld``) merge the vertices with equal values into the lowest one and
drop unreferenced vertices and dropped triangles: the mesh for readers that trust indices (``extract_surface(weld=True)``).

``smooth_meshes`` / ``Mesh.smoothed`` / ``Mesh.vertex_normals`` / ``Mesh.incidence`` (``pr_mesh_smooth``) are that reader: vertex-to-
triangle incidence lists, Laplacian / Taubin smoothing on them and area-weighted vertex normals of the result, deterministic bit for
bit (``extract_surface(smooth=n)``).

``sample_meshes`` / ``Mesh.sample`` / ``RayGrid.sample`` (``pr_mesh_sample``) draw points on the surfaces with probability proportional
to area - repeatable bit for bit from a seed, with normals and feature rows carried to the points - and ``compare_meshes`` measures
with them how far one mesh lies from another as a surface integral (mean, rms, max, Chamfer distance, F-score), where
``Mesh.distance_to`` looks from the vertices only.

``RayGrid.intersect`` / ``Mesh.intersections`` / ``Mesh.self_intersections`` / ``collide`` (``pr_mesh_intersect``) find on the same
grid the triangle pairs in which a second mesh, posed by a transform, cuts the grid's mesh - or a mesh cuts itself -, with one contact
segment per pair: the results of the exhaustive rule over all pairs, bit for bit, whatever the grid.
"""
from __future__ import annotations

import ctypes as C
import math
import operator
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib
from .field_query import NO_CPU


@dataclass
class Mesh:
    """``vertices (V, 3)`` fp32, ``triangles (T, 3)`` int32 into them, ``normals (V, 3)`` unit vectors toward falling density (zero
    rows where the lattice gradient vanishes or is not finite) or None, ``features (V, F)`` or None."""
    vertices: torch.Tensor
    triangles: torch.Tensor
    normals: Optional[torch.Tensor] = None
    features: Optional[torch.Tensor] = None

    def transformed(self, matrix: torch.Tensor) -> "Mesh":
        """A copy under the 4x4 (or 3x4) rigid transformation ``matrix`` (e.g. object-to-world): ``v' = R v + t``, normals are
        rotated by ``R``; triangles and features are shared."""
        m = torch.as_tensor(matrix, dtype=torch.float32, device=self.vertices.device)
        if m.dim() != 2 or m.size(1) != 4 or m.size(0) not in (3, 4):
            raise ValueError(f"matrix must be (4, 4) or (3, 4), got {list(m.shape)}")
        rotation, translation = m[:3, :3], m[:3, 3]
        normals = None if self.normals is None else self.normals @ rotation.T
        return Mesh(self.vertices @ rotation.T + translation, self.triangles, normals, self.features)

    def save_obj(self, path) -> None:
        """Writes a Wavefront OBJ file: ``v`` lines, ``vn`` lines when the mesh has normals, ``f`` lines (1-based; ``a//a`` with
        normals).  A plain host writer: the tensors are read back."""
        v = self.vertices.detach().cpu().tolist()
        n = None if self.normals is None else self.normals.detach().cpu().tolist()
        with open(path, "w") as f:
            f.write(f"# {len(v)} vertices, {self.triangles.size(0)} triangles\n")
            f.writelines("v %.9g %.9g %.9g\n" % tuple(row) for row in v)
            if n is not None:
                f.writelines("vn %.9g %.9g %.9g\n" % tuple(row) for row in n)
            for a, b, c in (self.triangles.detach().cpu() + 1).tolist():
                f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n" if n is not None else f"f {a} {b} {c}\n")

    def simplified(self, origin, cell, cells, **kw) -> "Mesh":
        """The mesh clustered on the grid ``origin`` / ``cell`` / ``cells``: ``simplify_meshes`` of this one mesh."""
        return simplify_meshes([self], origin, cell, cells, **kw)[0]

    def ray_grid(self, origin, cell, cells) -> "RayGrid":
        """This one mesh sorted into the grid ``origin`` / ``cell`` / ``cells`` for ray queries: ``RayGrid.build([self], ...)``."""
        return RayGrid.build([self], origin, cell, cells)

    def distance_to(self, other, *, max_distance: float, cells=32) -> torch.Tensor:
        """The distance ``(V)`` of every vertex of this mesh from ``other`` - a ``RayGrid`` of one group, or a ``Mesh``, which is
        sorted into ``bounding_grid([other], cells)`` first - within ``max_distance`` (``+inf`` beyond it): the one-sided deviation of
        this mesh from the other, e.g. of a simplified mesh from the one it came from (``RayGrid.closest``)."""
        if isinstance(other, Mesh):
            other = RayGrid.build([other], *bounding_grid([other], cells))
        if other.groups != 1:
            raise ValueError(f"distance_to needs a grid of one group, got {other.groups}")
        return other.closest(self.vertices, max_distance=max_distance).distance[0]

    def intersections(self, other, *, transform=None, cells=32, **kw) -> "MeshContacts":
        """The triangles of this mesh, posed by ``transform`` (into the other's frame; None: as it is), that cut ``other`` - a
        ``RayGrid`` of one group, or a ``Mesh``, which is sorted into ``bounding_grid([other], cells)`` first:
        ``RayGrid.intersect([self], transform=transform, **kw)[0]`` (``pairs=True`` / ``segments=True`` for the pairs and the contact
        segments)."""
        if isinstance(other, Mesh):
            if not (self.vertices.is_cuda and other.vertices.is_cuda):
                raise RuntimeError(NO_CPU)
            other = RayGrid.build([other], *bounding_grid([other], cells))
        if other.groups != 1:
            raise ValueError(f"intersections needs a grid of one group, got {other.groups}")
        return other.intersect([self], transform=transform, **kw)[0]

    def self_intersections(self, *, cells=32, pairs: bool = False) -> "MeshContacts":
        """Where this mesh cuts itself - what ``simplified`` (two sheets can meet in a cell) and many ``smoothed`` iterations can
        cause, and what ``audit()`` does not see: the mesh on ``bounding_grid([self], cells)`` against itself
        (``RayGrid.intersect(self_=True)``).  Triangles that share a corner value are no pair; ``report()["pairs"]`` counts every
        unordered pair once.  ``contains``, ``signed_volume`` and ``compare_meshes`` mean what they say only where this is 0."""
        if not (self.vertices.is_cuda and self.triangles.is_cuda):
            raise RuntimeError(NO_CPU)
        return RayGrid.build([self], *bounding_grid([self], cells)).intersect(self_=True, pairs=pairs)[0]

    def audit(self, labels: bool = False) -> "MeshAudit":
        """How this one mesh is made up: ``audit_meshes([self], labels=labels)[0]``.  A welded mesh (``welded``) answers
        identically, except that it has no dropped triangles."""
        return audit_meshes([self], labels=labels)[0]

    def welded(self, **kw):
        """This one mesh with one vertex per value, no unreferenced vertex and no dropped triangle: ``weld_meshes([self], **kw)``,
        the mesh itself - or, with ``maps=True``, the triple ``(mesh, vertex_map, triangle_map)``."""
        if kw.get("maps"):
            meshes, vertex_maps, triangle_maps = weld_meshes([self], **kw)
            return meshes[0], vertex_maps[0], triangle_maps[0]
        return weld_meshes([self], **kw)[0]

    def compacted(self) -> "Mesh":
        """This one mesh without its unreferenced vertices and its dropped triangles; no vertices are merged:
        ``weld_meshes([self], merge=False)[0]``."""
        return weld_meshes([self], merge=False)[0]

    def smoothed(self, **kw):
        """This one mesh after Taubin smoothing: ``smooth_meshes([self], **kw)``, the mesh itself - or, with ``report=True``, the
        triple ``(mesh, counts, state)``.  Welds first unless ``weld=False``."""
        if kw.get("report"):
            meshes, counts, states = smooth_meshes([self], **kw)
            return meshes[0], counts[0], states[0]
        return smooth_meshes([self], **kw)[0]

    def vertex_normals(self, **kw) -> "Mesh":
        """The same vertices, triangles and features with the normals recomputed from the triangles - area-weighted, pointing where the
        triangles point: ``smooth_meshes`` with no step and no weld.  What a mesh wants after ``simplified``, whose normals are still
        the lattice gradients at the representatives' old positions.  Identity is by index: a vertex of an unwelded mesh gets the
        normal of its own triangles only.  ``max_degree`` is ``smooth_meshes``'s."""
        return smooth_meshes([self], iterations=0, weld=False, normals=True, **kw)[0]

    def sample(self, n: int, *, seed: int, **kw) -> "SurfaceSamples":
        """``n`` points on this one mesh, drawn with probability proportional to area: ``sample_meshes([self], n, seed=seed, **kw)[0]``."""
        return sample_meshes([self], n, seed=seed, **kw)[0]

    def incidence(self, max_degree: int = 64):
        """The vertex-to-triangle incidence lists of this mesh as a CSR: ``(offsets (V + 1), triangles)`` int32 - the valid triangles
        (three different indices in range, nine finite coordinates) with a corner at vertex ``v`` are
        ``triangles[offsets[v]:offsets[v + 1]]``, ascending (a list longer than ``max_degree`` holds the right set in an unspecified
        order).  ``triangles`` has room for ``3 T`` entries, of which ``offsets[V]`` are written; nothing is read back."""
        if not (self.vertices.is_cuda and self.triangles.is_cuda):
            raise RuntimeError(NO_CPU)
        _, _, _, max_degree = _smooth_arguments(0, 0.0, None, max_degree)
        out = _smooth_packed(_pack_meshes([self], self.vertices.device), steps=0, lam=0.0, mu=0.0, max_degree=max_degree,
                             pin_border=True, normals=False, incidence=True)
        return out["incidence_offsets"], out["incidence"][:3 * self.triangles.size(0)]

    def keep_shells(self, n: int, compact: bool = False) -> "Mesh":
        """The mesh restricted to its ``n`` largest shells by triangle count (ties: the lower label first; ``MeshAudit.labels``):
        floater removal AFTER simplification, which can detach fragments that ``clean_lattice`` never saw.  Dropped triangles (an
        index out of range, a vertex that is not finite, ``a == b`` or ``a == c`` as values) belong to no shell and go.  The
        triangles that stay keep their order; vertices, normals and features are kept whole, as the simplifier keeps unreferenced
        vertices.  One audit, a ``bincount`` / ``topk`` over its labels and a boolean selection, which reads the number of kept
        triangles back: ONE host synchronisation.  ``compact=True``: the result then goes through ``compacted()``, which drops the
        vertex, normal and feature rows that no kept triangle refers to (one more synchronisation; features come back as fp32)."""
        if compact:
            return self.keep_shells(n).compacted()
        try:
            n = operator.index(n)
        except TypeError:
            raise ValueError(f"n must be an integer >= 1, got {n!r}") from None
        if n < 1:
            raise ValueError(f"n must be an integer >= 1, got {n}")
        labels = self.audit(labels=True).labels.to(torch.int64)
        T = labels.numel()
        if T == 0:
            return Mesh(self.vertices, self.triangles, self.normals, self.features)
        candidate = labels >= 0
        sizes = torch.bincount(labels[candidate], minlength=T)                # (at the shell's label, its lowest triangle)
        index = torch.arange(T, device=labels.device)
        key = torch.where(sizes > 0, sizes * (T + 1) + (T - index), torch.zeros_like(sizes))      # size first, then the lower label
        best = torch.topk(key, min(n, T)).indices
        kept_label = torch.zeros(T, dtype=torch.bool, device=labels.device)
        kept_label[best] = sizes[best] > 0
        keep = candidate & kept_label[labels.clamp(min=0)]
        return Mesh(self.vertices, self.triangles[keep], self.normals, self.features)


@dataclass
class _PackedMeshes:
    """G meshes as the library reads them: ``vertices (max(V, 1), 3)`` fp32 and ``triangles (max(T, 1), 3)`` int32, concatenated,
    contiguous, on one device; the host lists ``vo`` / ``to`` of G + 1 running offsets into them; ``V = vo[G]``, ``T = to[G]``;
    ``normals (max(V, 1), 3)`` and ``attributes (max(V, 1), A)`` fp32 or None.  ``_packed`` makes one and states the rule for the
    rows beyond V and T."""
    vertices: torch.Tensor
    triangles: torch.Tensor
    vo: List[int]
    to: List[int]
    V: int
    T: int
    normals: Optional[torch.Tensor] = None
    attributes: Optional[torch.Tensor] = None

    @property
    def groups(self) -> int:
        return len(self.vo) - 1

    def arguments(self):
        """What every mesh description starts with - ``(vertices, triangles, vertex_offsets, triangle_offsets, V, T)`` - with the two
        offset arrays as the rows of one new ``(2, G + 1)`` int32 device tensor."""
        offsets = torch.tensor([self.vo, self.to], dtype=torch.int32).to(self.vertices.device)
        return self.vertices, self.triangles, offsets[0], offsets[1], self.V, self.T


def _packed(vertices, triangles, vo, to, normals=None, attributes=None) -> _PackedMeshes:
    """The record of arrays that are packed already (``vo`` / ``to``: host lists).  THE PLACEHOLDER RULE: an empty tensor has no
    address and the library refuses NULL for an input array, so with V == 0 every per-vertex array that is given - vertices, normals,
    attributes - and with T == 0 the triangles are replaced by one uninitialised row, which nothing reads because the totals stay 0.
    Outputs are the caller's: each site sizes them by its own rule."""
    dev = vertices.device
    if vo[-1] == 0:
        vertices, normals, attributes = [None if x is None else torch.empty((1, x.size(1)), dtype=torch.float32, device=dev)
                                         for x in (vertices, normals, attributes)]
    if to[-1] == 0:
        triangles = torch.empty((1, 3), dtype=torch.int32, device=dev)
    return _PackedMeshes(vertices, triangles, vo, to, vo[-1], to[-1], normals, attributes)


def _mesh_shapes(meshes) -> None:
    for m in meshes:
        if m.vertices.dim() != 2 or m.vertices.size(1) != 3 or m.triangles.dim() != 2 or m.triangles.size(1) != 3:
            raise ValueError(f"a mesh has vertices (V, 3) and triangles (T, 3), got {list(m.vertices.shape)} / {list(m.triangles.shape)}")


def _pack_meshes(meshes, dev, *, normals: bool = False, features: Optional[int] = None) -> _PackedMeshes:
    """The meshes of a non-empty list concatenated on ``dev`` as fp32 / int32 rows - whatever their dtype - with their running
    offsets (``_packed``).  ``normals``: the ``Mesh.normals`` too.  ``features``: their common width (``_feature_width``) - the
    ``Mesh.features`` as fp32 attribute rows, none at width 0.  Pure torch: CPU tensors pack as device tensors do."""
    _mesh_shapes(meshes)
    pack = lambda parts, dtype, width=3: torch.cat([p.detach().to(device=dev, dtype=dtype).reshape(-1, width) for p in parts]).contiguous()
    vertices = pack([m.vertices for m in meshes], torch.float32)
    triangles = pack([m.triangles for m in meshes], torch.int32)
    rows = pack([m.normals for m in meshes], torch.float32) if normals else None
    if rows is not None and rows.size(0) != vertices.size(0):
        raise ValueError("normals must have one row per vertex")
    attributes = None
    if features is not None:
        if any(m.features.size(0) != m.vertices.size(0) for m in meshes):
            raise ValueError("features must have one row per vertex")
        attributes = pack([m.features for m in meshes], torch.float32, features) if features else None
    vo, to = [0], [0]
    for m in meshes:
        vo.append(vo[-1] + m.vertices.size(0))
        to.append(to[-1] + m.triangles.size(0))
    return _packed(vertices, triangles, vo, to, rows, attributes)


def _feature_width(meshes, cap: int) -> Optional[int]:
    """The width of the meshes' feature rows where EVERY mesh has ``(V, F)`` features with one common F - 0 included: the caller
    says what no columns mean -, else None.  More than ``cap`` columns raise."""
    if not all(m.features is not None and m.features.dim() == 2 for m in meshes) or len({m.features.size(1) for m in meshes}) != 1:
        return None
    width = meshes[0].features.size(1)
    if width > cap:
        raise ValueError(f"features can be at most {cap} wide, got {width}")
    return width


def _listed(meshes, who: str) -> List[Mesh]:
    meshes = list(meshes)
    if not meshes:
        raise ValueError(f"{who} needs at least one mesh")
    return meshes


def _device_of(meshes):
    if not all(m.vertices.is_cuda and m.triangles.is_cuda for m in meshes):
        raise RuntimeError(NO_CPU)
    return meshes[0].vertices.device


def _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, flags: int = 0) -> None:
    s.groups = vertex_offsets.numel() - 1
    s.total_vertices = int(total_vertices)
    s.total_triangles = int(total_triangles)
    s.flags = flags


def _set_grid(s, origin, cell, cells) -> None:
    for a in range(3):
        s.origin[a] = float(origin[a])
        s.cell[a] = float(cell[a])
        s.cells[a] = int(cells[a])


def _set_pointers(s, **tensors):
    """The pointer fields of a description by name: the tensor's address, NULL for None.  Returns the description."""
    for name, t in tensors.items():
        setattr(s, name, None if t is None else t.data_ptr())
    return s


def _call(name: str, description, workspace: torch.Tensor, size: int, dev) -> None:
    """One library call with a workspace, on the current stream of ``dev``."""
    _lib.check(getattr(_lib.load(), name)(C.byref(description), workspace.data_ptr(), size, torch.cuda.current_stream(dev).cuda_stream),
               name)


def _call_with_workspace(size_name: str, name: str, description, dev):
    """Asks ``size_name`` what ``description`` needs, allocates it on ``dev`` and makes the call ``name`` with it.  Returns
    ``(workspace, size)`` for the count-then-emit sites, whose second ``_call`` uses the same workspace."""
    size = C.c_size_t()
    _lib.check(getattr(_lib.load(), size_name)(C.byref(description), C.byref(size)), size_name)
    workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
    _call(name, description, workspace, size.value, dev)
    return workspace, size.value


def surface_struct(sigma: torch.Tensor, axes: Sequence[torch.Tensor], level: float, vertex_offsets: torch.Tensor,
                   triangle_offsets: torch.Tensor, vertices: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                   triangles: Optional[torch.Tensor] = None) -> _lib.Surface:
    """``pr_surface_t`` over prepared tensors (fp32 / int32, contiguous, one device); the capacities are the outputs' rows."""
    s = _lib.Surface()
    s.groups = sigma.size(0)
    for a in range(3):
        s.points[a] = sigma.size(1 + a)
        s.axis[a] = axes[a].data_ptr()
    s.level = float(level)
    s.max_vertices = 0 if vertices is None else vertices.size(0)
    s.max_triangles = 0 if triangles is None else triangles.size(0)
    return _set_pointers(s, sigma=sigma, vertices=vertices, normals=normals, triangles=triangles, vertex_offsets=vertex_offsets,
                         triangle_offsets=triangle_offsets)


def components_struct(sigma: torch.Tensor, level: float, counts: torch.Tensor, *, labels: Optional[torch.Tensor] = None,
                      sizes: Optional[torch.Tensor] = None, sigma_out: Optional[torch.Tensor] = None, keep_largest: int = 0,
                      min_points: int = 0, close_border: bool = False, fill: Optional[float] = None) -> _lib.Components:
    """``pr_components_t`` over prepared tensors (fp32 / int32, contiguous, one device); ``fill=None`` means ``level``."""
    c = _lib.Components()
    c.groups = sigma.size(0)
    for a in range(3):
        c.points[a] = sigma.size(1 + a)
    c.level = float(level)
    c.flags = _lib.COMPONENTS_CLOSE_BORDER if close_border else 0
    c.min_points = int(min_points)
    c.keep_largest = int(keep_largest)
    c.fill = float(level if fill is None else fill)
    return _set_pointers(c, sigma=sigma, labels=labels, sizes=sizes, sigma_out=sigma_out, counts=counts)


def _lattice(sigma: torch.Tensor) -> torch.Tensor:
    if not sigma.is_cuda:
        raise RuntimeError(NO_CPU)
    if sigma.dim() != 4:
        raise ValueError(f"sigma must be (G, nx, ny, nz), got {list(sigma.shape)}")
    return sigma.detach().to(torch.float32).contiguous()


def _run_components(sigma: torch.Tensor, level: float, **outputs) -> torch.Tensor:
    """One ``pr_label_components`` call on the current stream of ``sigma``'s device; returns ``counts (G, 4)``."""
    dev = sigma.device
    with torch.cuda.device(dev):
        counts = torch.empty((sigma.size(0), 4), dtype=torch.int32, device=dev)
        _call_with_workspace("pr_components_workspace_size", "pr_label_components", components_struct(sigma, level, counts, **outputs), dev)
    return counts


def label_components(sigma: torch.Tensor, level: float, *, close_border: bool = False):
    """Connected components of the inside set ``sigma > level`` of ``sigma (G, nx, ny, nz)`` under the 14-neighbourhood of the
    mesher's seven edge directions (``pr_label_components``, include/playrender.h).  Returns ``(labels, sizes, counts)`` on the
    device: int32 ``(G, nx, ny, nz)`` labels (the smallest flat index of the point's component inside its group, -1 outside) and
    sizes (points of the point's component, 0 outside), and ``counts (G, 4)`` = inside points, components, kept components, kept
    points.  ``close_border``: the border layer of the lattice counts as outside.  No host synchronisation."""
    sigma = _lattice(sigma)
    labels = torch.empty(sigma.shape, dtype=torch.int32, device=sigma.device)
    sizes = torch.empty(sigma.shape, dtype=torch.int32, device=sigma.device)
    counts = _run_components(sigma, level, labels=labels, sizes=sizes, close_border=close_border)
    return labels, sizes, counts


def clean_lattice(sigma: torch.Tensor, level: float, *, keep_largest: int = 0, min_points: int = 0, close_border: bool = False,
                  fill: Optional[float] = None):
    """``sigma`` with its unwanted components blanked out: ``(sigma_out, counts)``.  The components of every group are ranked by size
    (ties: the smaller label first); one is kept iff it has at least ``min_points`` points and - with ``keep_largest`` in 1..8 - is
    among the ``keep_largest`` largest.  Every inside point of a component that is not kept holds ``fill`` (``None``: ``level``, which
    is outside) and, with ``close_border``, so does every border point ``> level``; all other values are the input's, bit for bit.
    ``counts (G, 4)`` as in ``label_components``.  No host read-back."""
    if not 0 <= int(keep_largest) <= _lib.COMPONENTS_MAX_KEEP:
        raise ValueError(f"keep_largest must be in 0..{_lib.COMPONENTS_MAX_KEEP}, got {keep_largest}")
    if int(min_points) < 0:
        raise ValueError(f"min_points must be >= 0, got {min_points}")
    if fill is not None and not float(fill) <= float(level):
        raise ValueError(f"fill must be <= level ({level}), got {fill}")
    sigma = _lattice(sigma)
    out = torch.empty_like(sigma)
    counts = _run_components(sigma, level, sigma_out=out, keep_largest=keep_largest, min_points=min_points, close_border=close_border,
                             fill=fill)
    return out, counts


def skeleton_indices(n: int, stride: int) -> List[int]:
    """The skeleton indices of an axis of ``n`` lattice points (``pr_band_t``): ``0, stride, 2 stride, ...`` below ``n``, plus
    ``n - 1`` if it is not among them."""
    n, stride = int(n), int(stride)
    if n < 2:
        raise ValueError(f"a lattice has at least 2 points per axis, got {n}")
    if not _lib.BAND_MIN_STRIDE <= stride <= _lib.BAND_MAX_STRIDE:
        raise ValueError(f"stride must be in {_lib.BAND_MIN_STRIDE}..{_lib.BAND_MAX_STRIDE}, got {stride}")
    idx = list(range(0, n, stride))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return idx


def band_struct(sigma: torch.Tensor, axes: Sequence[torch.Tensor], level: float, stride: int, guard: int, point_offsets: torch.Tensor,
                counts: torch.Tensor, *, active: Optional[torch.Tensor] = None, point_index: Optional[torch.Tensor] = None,
                positions: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None, exact: Optional[torch.Tensor] = None,
                max_points: Optional[int] = None) -> _lib.Band:
    """``pr_band_t`` over prepared tensors (fp32 / int32 / uint8, contiguous, one device); ``max_points=None``: the rows of the first
    of ``point_index``, ``positions``, ``values`` that is given (0 without any)."""
    b = _lib.Band()
    b.groups = sigma.size(0)
    for a in range(3):
        b.points[a] = sigma.size(1 + a)
        b.axis[a] = axes[a].data_ptr()
    b.level = float(level)
    b.stride = int(stride)
    b.guard = int(guard)
    if max_points is None:
        rows = [t.size(0) for t in (point_index, positions, values) if t is not None]
        max_points = rows[0] if rows else 0
    b.max_points = int(max_points)
    some = lambda t: None if t is None or t.numel() == 0 else t       # (the band's own rule: an optional array without elements is NULL)
    return _set_pointers(b, sigma=sigma, point_offsets=point_offsets, counts=counts, active=some(active),
                         point_index=some(point_index), positions=some(positions), values=some(values), exact=some(exact))


def refine_band(sigma: torch.Tensor, axes: Sequence[torch.Tensor], level: float, *, stride: int, guard: int = 1, evaluate):
    """Fills a lattice of which only the skeleton is known, spending ``evaluate`` only in a band around the level set
    (``pr_band_plan`` / ``pr_band_fill``, include/playrender.h).

    ``sigma (G, nx, ny, nz)`` (device tensor, z fastest) holds the field at its skeleton points - ``skeleton_indices`` per axis, every
    ``stride``-th point and the last; all other entries are ignored.  A skeleton cell whose 8 corners are not all on one side of
    ``level`` is mixed; every non-skeleton point of a cell within ``guard`` cells of a mixed one is evaluated:
    ``evaluate(g, positions (M, 3)) -> (M,)`` is the caller's field for group ``g`` (called for the groups that have points).  Every other
    point receives a copy of a skeleton value of its cell, which is on the right side of ``level`` as far as the skeleton can tell.

    AN APPROXIMATION: a feature thinner than ``stride`` that no skeleton cell sees as mixed is lost, whatever ``guard`` is.  With
    ``guard >= 1`` and a surface the skeleton does see, the mesh of the result (positions, triangles and normals) is the mesh of the
    dense lattice.

    Three calls on the current stream: a counting plan call, then - after reading ``point_offsets`` back, the ONE host
    synchronisation of this function - an emitting one into exactly sized tensors, the evaluations, the fill.  Returns
    ``(sigma, exact, counts)``: the filled lattice (a new tensor), ``exact (G, nx, ny, nz)`` uint8 - 1 where the value is the field's
    own (skeleton and band), 0 where it is a copy - and ``counts (G, 4)`` int32 = cells, mixed cells, active cells, band points."""
    if not sigma.is_cuda:
        raise RuntimeError(NO_CPU)
    if sigma.dim() != 4:
        raise ValueError(f"sigma must be (G, nx, ny, nz), got {list(sigma.shape)}")
    if len(axes) != 3:
        raise ValueError("axes must be the three coordinate vectors of the lattice")
    if not _lib.BAND_MIN_STRIDE <= int(stride) <= _lib.BAND_MAX_STRIDE:
        raise ValueError(f"stride must be in {_lib.BAND_MIN_STRIDE}..{_lib.BAND_MAX_STRIDE}, got {stride}")
    if not 0 <= int(guard) <= _lib.BAND_MAX_GUARD:
        raise ValueError(f"guard must be in 0..{_lib.BAND_MAX_GUARD}, got {guard}")
    dev = sigma.device
    sigma = sigma.detach().to(torch.float32).contiguous().clone()
    axes = [torch.as_tensor(a).detach().to(device=dev, dtype=torch.float32).contiguous() for a in axes]
    for a in range(3):
        if axes[a].dim() != 1 or axes[a].numel() != sigma.size(1 + a):
            raise ValueError(f"axes[{a}] must hold {sigma.size(1 + a)} coordinates, got {list(axes[a].shape)}")
    G = sigma.size(0)
    with torch.cuda.device(dev):
        point_offsets = torch.empty(G + 1, dtype=torch.int32, device=dev)
        counts = torch.empty((G, 4), dtype=torch.int32, device=dev)
        count = band_struct(sigma, axes, level, stride, guard, point_offsets, counts)
        workspace, size = _call_with_workspace("pr_band_workspace_size", "pr_band_plan", count, dev)
        offsets = point_offsets.cpu().tolist()                               # (the host synchronisation)
        rows = offsets[G]
        positions = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        values = torch.empty(rows, dtype=torch.float32, device=dev)
        if rows > 0:
            emit = band_struct(sigma, axes, level, stride, guard, point_offsets, counts, positions=positions)
            _call("pr_band_plan", emit, workspace, size, dev)
            for g in range(G):
                if offsets[g + 1] > offsets[g]:
                    got = evaluate(g, positions[offsets[g]:offsets[g + 1]])
                    if got.numel() != offsets[g + 1] - offsets[g]:
                        raise ValueError(f"evaluate({g}, ...) returned {list(got.shape)} for {offsets[g + 1] - offsets[g]} positions")
                    values[offsets[g]:offsets[g + 1]] = got.detach().reshape(-1).to(device=dev, dtype=torch.float32)
        exact = torch.empty(sigma.shape, dtype=torch.uint8, device=dev)
        fill = band_struct(sigma, axes, level, stride, guard, point_offsets, counts, values=values, exact=exact)
        _call("pr_band_fill", fill, workspace, size, dev)
    return sigma, exact, counts


def simplify_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                    total_vertices: int, total_triangles: int, origin, cell, cells, counts: torch.Tensor, out_vertex_offsets: torch.Tensor,
                    out_triangle_offsets: torch.Tensor, *, normals: Optional[torch.Tensor] = None,
                    out_vertices: Optional[torch.Tensor] = None, out_normals: Optional[torch.Tensor] = None,
                    out_triangles: Optional[torch.Tensor] = None, vertex_map: Optional[torch.Tensor] = None,
                    keep_duplicates: bool = False) -> _lib.Simplify:
    """``pr_simplify_t`` over prepared tensors (fp32 / int32, contiguous, one device); the capacities are the outputs' rows."""
    s = _lib.Simplify()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, _lib.SIMPLIFY_KEEP_DUPLICATES if keep_duplicates else 0)
    _set_grid(s, origin, cell, cells)
    s.max_vertices = 0 if out_vertices is None else out_vertices.size(0)
    s.max_triangles = 0 if out_triangles is None else out_triangles.size(0)
    return _set_pointers(s, vertices=vertices, normals=normals, triangles=triangles, vertex_offsets=vertex_offsets,
                         triangle_offsets=triangle_offsets, out_vertices=out_vertices, out_normals=out_normals,
                         out_triangles=out_triangles, vertex_map=vertex_map, counts=counts, out_vertex_offsets=out_vertex_offsets,
                         out_triangle_offsets=out_triangle_offsets)


def _cluster_grid(origin, cell, cells):
    """The host values of a cluster grid, checked as ``pr_simplify_mesh`` checks them."""
    try:
        origin, cell, cells = [float(x) for x in origin], [float(x) for x in cell], [operator.index(x) for x in cells]
    except TypeError:
        raise ValueError("origin and cell must be three numbers each, cells three integers") from None
    if not len(origin) == len(cell) == len(cells) == 3:
        raise ValueError("origin, cell and cells must have three entries each")
    if not all(math.isfinite(x) for x in origin):
        raise ValueError(f"origin must be finite, got {origin}")
    if not all(math.isfinite(x) and x > 0 for x in cell):
        raise ValueError(f"cell sizes must be finite and > 0, got {cell}")
    if not all(n >= 1 for n in cells) or cells[0] * cells[1] * cells[2] > _lib.SIMPLIFY_MAX_CELLS:
        raise ValueError(f"cells must be >= 1 per axis with a product of at most 2^21 = {_lib.SIMPLIFY_MAX_CELLS}, got {cells}")
    return origin, cell, cells


def lattice_cluster_grid(axes: Sequence, k: int):
    """The cluster grid aligned with a lattice, ``k`` lattice steps per cell: per axis ``origin = axes[a][0]``,
    ``cell = k (axes[a][-1] - axes[a][0]) / (n_a - 1)``, ``cells = ceil((n_a - 1) / k)``.  Reads the ends of the axes back."""
    k = operator.index(k)
    if k < 1:
        raise ValueError(f"the cells of a lattice-aligned grid span k >= 1 lattice steps, got {k}")
    origin, cell, cells = [], [], []
    for a in axes:
        a = torch.as_tensor(a).detach().to(torch.float32).reshape(-1)
        if a.numel() < 2:
            raise ValueError("a lattice has at least 2 points per axis")
        first, last = a[[0, -1]].cpu().tolist()
        origin.append(first)
        cell.append(k * (last - first) / (a.numel() - 1))
        cells.append(-(-(a.numel() - 1) // k))
    return origin, cell, cells


def _simplify_packed(p: _PackedMeshes, origin, cell, cells, keep_duplicates, placement: str = "mean"):
    """``pr_simplify_mesh`` on packed meshes: a counting call, one read-back of the two offset arrays, an exactly sized emitting
    call.  ``placement="quadric"``: the emitting call also writes its vertex map and ONE ``pr_mesh_place`` call follows on the same
    stream, with ``scale = max(cell)`` and ``max_move = cell`` - nothing more is read back.  Returns the list of meshes."""
    dev, G = p.vertices.device, p.groups
    quadric = _placement(placement)
    with torch.cuda.device(dev):
        offsets = torch.empty((2, G + 1), dtype=torch.int32, device=dev)
        counts = torch.empty((G, 4), dtype=torch.int32, device=dev)
        mesh = p.arguments()
        common = (*mesh, origin, cell, cells, counts, offsets[0], offsets[1])
        count = simplify_struct(*common, normals=p.normals, keep_duplicates=keep_duplicates)
        workspace, size = _call_with_workspace("pr_simplify_workspace_size", "pr_simplify_mesh", count, dev)
        out_vo, out_to = offsets.cpu().tolist()                             # (the host synchronisation)
        out_v = torch.empty((out_vo[G], 3), dtype=torch.float32, device=dev)
        out_n = None if p.normals is None else torch.empty((out_vo[G], 3), dtype=torch.float32, device=dev)
        out_t = torch.empty((out_to[G], 3), dtype=torch.int32, device=dev)
        if out_vo[G] > 0:
            vertex_map = torch.empty(p.V, dtype=torch.int32, device=dev) if quadric else None
            emit = simplify_struct(*common, normals=p.normals, out_vertices=out_v, out_normals=out_n,
                                   out_triangles=out_t if out_to[G] > 0 else None, vertex_map=vertex_map,
                                   keep_duplicates=keep_duplicates)
            _call("pr_simplify_mesh", emit, workspace, size, dev)
            if quadric:
                placed = torch.empty_like(out_v)
                s = place_struct(*mesh, vertex_map, out_v, offsets[0], out_vo[G], placed,
                                 torch.empty((G, _lib.PLACE_COUNTS), dtype=torch.int32, device=dev), scale=max(cell), max_move=cell,
                                 merged_triangles=out_t if out_to[G] > 0 else None,
                                 merged_triangle_offsets=offsets[1] if out_to[G] > 0 else None, total_merged_triangles=out_to[G])
                _call_with_workspace("pr_mesh_place_workspace_size", "pr_mesh_place", s, dev)
                out_v = placed
    return [Mesh(out_v[out_vo[g]:out_vo[g + 1]], out_t[out_to[g]:out_to[g + 1]], None if out_n is None else out_n[out_vo[g]:out_vo[g + 1]])
            for g in range(G)]


PLACEMENTS = ("mean", "quadric")
PLACE_REGULARISATION = 2.0 ** -10


def _placement(placement) -> bool:
    """Whether ``placement`` asks for the quadric rule; anything but the two names raises."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, got {placement!r}")
    return placement == "quadric"


def simplify_meshes(meshes: Sequence[Mesh], origin, cell, cells, *, keep_duplicates: bool = False, placement: str = "mean") -> List[Mesh]:
    """The meshes simplified by vertex clustering on one uniform grid (``pr_simplify_mesh``, include/playrender.h): the grid has
    ``cells[a]`` cells of size ``cell[a]`` from ``origin[a]`` on along every axis (at most 2^21 cells); a vertex outside it goes to the
    nearest border cell.  All vertices of a cell become one vertex at their mean (normals: the normalised sum), triangles that lose a
    corner that way disappear, and of the triangles that end up with the same corners in the same orientation only the first stays
    (``keep_duplicates=True``: all stay).  The result is fixed by the rule - integer sums, no dependence on the execution order.

    ``placement="quadric"``: every cluster's vertex then moves from the mean to the point that minimises the area-weighted squared
    distance to the planes of the input triangles that touch the cluster (``pr_mesh_place`` with ``scale = max(cell)``,
    ``max_move = cell``, ``regularisation = 2^-10``; ``place_vertices`` is the call on its own): convex edges and corners stay where
    the surface has them instead of being pulled inwards.  One more call on the same stream, no further read-back; the triangle lists
    are the mean rule's, bit for bit, so edge balance and what ``contains`` and ``audit`` say of a ``keep_duplicates=True`` mesh hold.
    A few sliver triangles can turn over (``place_vertices`` counts them).  The normals stay the simplifier's normalised sums:
    ``Mesh.vertex_normals()`` recomputes them from the placed triangles.  ``"mean"`` (the default) is the call as it always was.

    The meshes are packed, counted, and - after reading the two offset arrays back, the ONE host synchronisation - emitted into
    exactly sized tensors.  Returns one mesh per input; they have normals iff every input has them; ``features`` are not carried
    over.  There is no CPU fallback."""
    meshes = _listed(meshes, "simplify_meshes")
    _placement(placement)
    dev = _device_of(meshes)
    origin, cell, cells = _cluster_grid(origin, cell, cells)
    p = _pack_meshes(meshes, dev, normals=all(m.normals is not None for m in meshes))
    return _simplify_packed(p, origin, cell, cells, keep_duplicates, placement)


def place_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                 total_vertices: int, total_triangles: int, vertex_map: torch.Tensor, merged_vertices: torch.Tensor,
                 merged_vertex_offsets: torch.Tensor, total_merged_vertices: int, out_vertices: torch.Tensor, counts: torch.Tensor, *,
                 scale: float, max_move, regularisation: float = PLACE_REGULARISATION, merged_triangles: Optional[torch.Tensor] = None,
                 merged_triangle_offsets: Optional[torch.Tensor] = None, total_merged_triangles: int = 0) -> _lib.MeshPlace:
    """``pr_mesh_place_t`` over prepared tensors (fp32 / int32, contiguous, one device)."""
    s = _lib.MeshPlace()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles)
    s.total_merged_vertices = int(total_merged_vertices)
    s.total_merged_triangles = int(total_merged_triangles)
    s.scale = float(scale)
    s.regularisation = float(regularisation)
    for a in range(3):
        s.max_move[a] = float(max_move[a])
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         vertex_map=vertex_map, merged_vertices=merged_vertices, merged_vertex_offsets=merged_vertex_offsets,
                         merged_triangles=merged_triangles, merged_triangle_offsets=merged_triangle_offsets, out_vertices=out_vertices,
                         counts=counts)


def _place_arguments(scale, max_move, regularisation):
    """``(scale, max_move, regularisation)`` checked as ``pr_mesh_place`` checks them."""
    try:
        scale, regularisation = float(scale), float(regularisation)
        max_move = [float(max_move)] * 3 if isinstance(max_move, (int, float)) else [float(x) for x in max_move]
    except TypeError:
        raise ValueError("scale and regularisation must be numbers, max_move one number or three") from None
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"scale must be finite and > 0, got {scale}")
    if not (math.isfinite(regularisation) and regularisation > 0):
        raise ValueError(f"regularisation must be finite and > 0, got {regularisation}")
    if len(max_move) != 3 or not all(math.isfinite(x) and x >= 0 for x in max_move):
        raise ValueError(f"max_move must be one or three finite numbers >= 0, got {max_move}")
    return scale, max_move, regularisation


def place_vertices(meshes: Sequence[Mesh], merged: Sequence[Mesh], vertex_maps, *, scale: float, max_move,
                   regularisation: float = PLACE_REGULARISATION):
    """The ``merged`` meshes - each a coarser version of the mesh of ``meshes`` at the same place, with ``vertex_maps[g] (V_g)`` the
    merged vertex of every vertex of ``meshes[g]`` (``pr_simplify_mesh``'s vertex map, ``weld_meshes(maps=True)``'s) - with every vertex
    moved to the minimum of its cluster's quadric (``pr_mesh_place``, include/playrender.h): the area-weighted squared distance to the
    planes of the triangles of ``meshes[g]`` with a corner in the cluster, plus ``regularisation`` times the mean diagonal of the
    quadric as a pull toward the stored position.  ``scale``: the unit of length in which the sums are taken, about a cluster's size
    (``max(cell)``); ``max_move``: one number or three, the largest move per axis - a vertex that would go further, or whose system
    cannot be solved, stays bit for bit.  Integer sums: the result does not depend on the execution order.

    Returns ``(meshes, counts)``: the merged meshes with new vertices - triangles shared, normals and features carried as they are -
    and the ``(G, 4)`` int32 counts on the device: vertices moved, vertices kept, contributions skipped plus invalid triangles,
    merged triangles that the move turned over.  One call, no host synchronisation.  There is no CPU fallback."""
    meshes, merged = _listed(meshes, "place_vertices"), list(merged)
    vertex_maps = list(vertex_maps)
    if not len(meshes) == len(merged) == len(vertex_maps):
        raise ValueError(f"place_vertices needs one merged mesh and one vertex map per mesh, got {len(meshes)} / {len(merged)} / {len(vertex_maps)}")
    scale, max_move, regularisation = _place_arguments(scale, max_move, regularisation)
    for m, vmap in zip(meshes, vertex_maps):
        if vmap.numel() != m.vertices.size(0):
            raise ValueError(f"a vertex map must have one entry per vertex of its mesh ({m.vertices.size(0)}), got {vmap.numel()}")
    dev = _device_of(meshes + merged)
    if not all(vmap.is_cuda for vmap in vertex_maps):
        raise RuntimeError(NO_CPU)
    fine, coarse = _pack_meshes(meshes, dev), _pack_meshes(merged, dev)
    G, VO, TO = fine.groups, coarse.V, coarse.T
    with torch.cuda.device(dev):
        vertex_map = torch.cat([vmap.detach().to(device=dev, dtype=torch.int32).reshape(-1) for vmap in vertex_maps]).contiguous()
        if fine.V == 0:
            vertex_map = torch.empty(1, dtype=torch.int32, device=dev)      # (the placeholder rule of _packed)
        merged_offsets = torch.tensor([coarse.vo, coarse.to], dtype=torch.int32).to(dev)
        out = torch.empty((max(VO, 1), 3), dtype=torch.float32, device=dev)
        counts = torch.empty((G, _lib.PLACE_COUNTS), dtype=torch.int32, device=dev)
        s = place_struct(*fine.arguments(), vertex_map, coarse.vertices, merged_offsets[0], VO, out, counts, scale=scale, max_move=max_move,
                         regularisation=regularisation, merged_triangles=coarse.triangles, merged_triangle_offsets=merged_offsets[1],
                         total_merged_triangles=TO)
        _call_with_workspace("pr_mesh_place_workspace_size", "pr_mesh_place", s, dev)
    return [Mesh(out[coarse.vo[g]:coarse.vo[g + 1]], m.triangles, m.normals, m.features) for g, m in enumerate(merged)], counts


def raycast_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                   total_vertices: int, total_triangles: int, origin, cell, cells, cell_offsets: torch.Tensor, *,
                   references: Optional[torch.Tensor] = None, origins: Optional[torch.Tensor] = None,
                   directions: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None, triangle: Optional[torch.Tensor] = None,
                   barycentric: Optional[torch.Tensor] = None, t_min: float = 0.0, t_max: float = math.inf,
                   cull_back: bool = False) -> _lib.Raycast:
    """``pr_raycast_t`` over prepared tensors (fp32 / int32, contiguous, one device); ``max_references`` is the rows of ``references``,
    ``rays`` the second dimension of ``origins (G, N, 3)``."""
    s = _lib.Raycast()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, _lib.RAYCAST_CULL_BACK if cull_back else 0)
    _set_grid(s, origin, cell, cells)
    s.max_references = 0 if references is None else references.size(0)
    s.rays = 0 if origins is None else origins.size(1)
    s.t_min = float(t_min)
    s.t_max = float(t_max)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         cell_offsets=cell_offsets, references=references, origins=origins, directions=directions, t=t,
                         triangle=triangle, barycentric=barycentric)


def _ray_grid(origin, cell, cells):
    """The host values of a ray grid, checked as ``pr_raycast_build`` checks them."""
    origin, cell, cells = _cluster_grid(origin, cell, cells)
    if not all(n <= _lib.RAYCAST_MAX_AXIS_CELLS for n in cells):
        raise ValueError(f"a ray grid has at most {_lib.RAYCAST_MAX_AXIS_CELLS} cells per axis, got {cells}")
    return origin, cell, cells


@dataclass
class RayHits:
    """What ``RayGrid.cast`` returns: ``t (G, N)`` (``+inf``: a miss), ``triangle (G, N)`` int32 local to the group (-1: a miss),
    ``barycentric (G, N, 2)`` = ``(u, v)`` of the hit (the point is ``a + u (b - a) + v (c - a)``) or None; with ``nearest=True``
    also ``nearest_t (N)`` and ``group (N)`` int64: the closest hit over the groups and the group it belongs to (-1: none hits)."""
    t: torch.Tensor
    triangle: torch.Tensor
    barycentric: Optional[torch.Tensor] = None
    nearest_t: Optional[torch.Tensor] = None
    group: Optional[torch.Tensor] = None


def _nearest_group(values: torch.Tensor, triangle: torch.Tensor):
    """The smallest of ``values (G, N)`` over the groups and the group it belongs to, -1 where that group found no triangle."""
    nearest, group = torch.min(values, dim=0)
    hit = triangle.gather(0, group.unsqueeze(0)).squeeze(0) >= 0
    return nearest, torch.where(hit, group, torch.full_like(group, -1))


class RayGrid:
    """G meshes sorted into a uniform cell grid for closest-hit ray queries (``pr_raycast_build`` / ``pr_raycast_query``,
    include/playrender.h).  ``RayGrid.build`` makes one; it holds the packed meshes, the per-cell lists and nothing else, and serves
    any number of ``cast`` calls.  The results are those of the exhaustive search over all triangles, bit for bit (the header states the
    domain of that guarantee).  There is no CPU fallback."""

    def __init__(self, vertices, triangles, vertex_offsets, triangle_offsets, totals, grid, cell_offsets, references):
        self.vertices, self.triangles = vertices, triangles
        self.vertex_offsets, self.triangle_offsets = vertex_offsets, triangle_offsets
        self.total_vertices, self.total_triangles = totals
        self.origin, self.cell, self.cells = grid
        self.cell_offsets, self.references = cell_offsets, references
        self.host_triangle_offsets = None                               # (``build`` knows them; ``_triangle_bounds`` reads them)

    @property
    def groups(self) -> int:
        return self.vertex_offsets.numel() - 1

    def _description(self):
        """The ten arguments every description of a query against this grid starts with."""
        return (self.vertices, self.triangles, self.vertex_offsets, self.triangle_offsets, self.total_vertices, self.total_triangles,
                self.origin, self.cell, self.cells, self.cell_offsets)

    @property
    def _references(self) -> Optional[torch.Tensor]:
        return self.references if self.references.numel() else None     # (a grid without references passes NULL)

    def _triangle_bounds(self) -> List[int]:
        """The G + 1 triangle offsets on the host; a grid that ``build`` did not make reads them back."""
        return self.host_triangle_offsets or self.triangle_offsets.cpu().tolist()

    def _group_points(self, x: torch.Tensor, what: str = "points") -> torch.Tensor:
        """``x (G, N, 3)``, or ``(N, 3)`` for every group, as fp32 ``(G, N, 3)`` on the grid's device."""
        G = self.groups
        if x.dim() not in (2, 3) or x.size(-1) != 3:
            raise ValueError(f"{what} must be (G, N, 3) or (N, 3), got {list(x.shape)}")
        if x.dim() == 3 and x.size(0) != G:
            raise ValueError(f"the grid holds {G} groups, the {what} are {list(x.shape)}")
        return (x if x.dim() == 3 else x.unsqueeze(0).expand(G, -1, -1)).detach().to(device=self.vertices.device, dtype=torch.float32).contiguous()

    @classmethod
    def build(cls, meshes: Sequence[Mesh], origin, cell, cells) -> "RayGrid":
        """Packs the meshes (``_pack_meshes``) and sorts their triangles into the grid of ``cells[a]`` cells of size ``cell[a]``
        from ``origin[a]`` on (at most 1024 per axis, 2^21 in all; ``bounding_grid`` and ``lattice_cluster_grid`` supply one): a
        counting call, one read-back of the number of references - the ONE host synchronisation - and an exactly sized emitting call.
        A triangle that is not inside the grid's box is tested by every ray: a grid around the meshes is the fast one."""
        meshes = _listed(meshes, "RayGrid.build")
        dev = _device_of(meshes)
        grid = _ray_grid(origin, cell, cells)
        p = _pack_meshes(meshes, dev)
        lists = p.groups * (grid[2][0] * grid[2][1] * grid[2][2] + 1)
        with torch.cuda.device(dev):
            mesh = p.arguments()
            cell_offsets = torch.empty(lists + 1, dtype=torch.int32, device=dev)
            workspace, size = _call_with_workspace("pr_raycast_workspace_size", "pr_raycast_build",
                                                   raycast_struct(*mesh, *grid, cell_offsets), dev)
            R = int(cell_offsets[lists].item())                                 # (the host synchronisation)
            if R < 0:
                raise RuntimeError("the grid holds 2^31 or more references: use a coarser grid")
            references = torch.empty(R, dtype=torch.int32, device=dev)
            if R > 0:
                _call("pr_raycast_build", raycast_struct(*mesh, *grid, cell_offsets, references=references), workspace, size, dev)
        made = cls(*mesh[:4], (p.V, p.T), grid, cell_offsets, references)
        made.host_triangle_offsets = p.to
        return made

    def audit(self, labels: bool = False) -> List["MeshAudit"]:
        """How the meshes this grid holds are made up (``pr_mesh_audit`` on the packed arrays, one ``MeshAudit`` per group): the
        question to ask before trusting ``contains`` - ``report()["balanced"]`` says whether every directed edge, by vertex value,
        occurs as often as its reverse.  One call on the current stream, no host synchronisation (``labels=True`` on a grid that
        was not made by ``build`` reads the triangle offsets back)."""
        if not self.vertices.is_cuda:
            raise RuntimeError(NO_CPU)
        counts, measures, shell = _audit_packed(*self._description()[:6], bool(labels))
        to = self._triangle_bounds() if labels else None
        return [MeshAudit(counts[g], measures[g], shell[to[g]:to[g + 1]] if labels else None) for g in range(self.groups)]

    def sample(self, n: int, *, seed: int, first: int = 0, normals: Optional[str] = "face") -> List["SurfaceSamples"]:
        """``n`` points on each of the meshes this grid holds, drawn with probability proportional to area (``pr_mesh_sample`` on the
        packed arrays, one ``SurfaceSamples`` per group; ``sample_meshes`` states the rule) - e.g. points to ``cast`` from or to test
        with ``contains``.  The grid holds positions only: ``normals`` is ``"face"`` or None.  One call on the current stream, no host
        synchronisation."""
        if normals not in ("face", None):
            raise ValueError(f"a RayGrid holds no vertex normals: normals must be 'face' or None, got {normals!r}")
        n, seed, first = _sample_arguments(n, seed, first, self.groups)
        if not self.vertices.is_cuda:
            raise RuntimeError(NO_CPU)
        return _surface_samples(_sample_packed(*self._description()[:6], n, seed, first, face=normals == "face"), self.groups)

    def cast(self, origins: torch.Tensor, directions: torch.Tensor, *, t_min: float = 0.0, t_max: float = math.inf,
             cull_back: bool = False, barycentric: bool = False, nearest: bool = False) -> RayHits:
        """The closest hit of every ray ``o + t d``, ``t_min <= t <= t_max``, with the meshes: ``origins`` / ``directions`` are
        ``(G, N, 3)`` - group g's rays meet group g's mesh - or ``(N, 3)``, used for every group; in the meshes' frame, not normalised.
        ``cull_back``: only triangles the ray meets from their front (it enters matter) count.  ``nearest``: also the closest hit over
        the groups - the cross-object front surface, as ``front_object`` is for renders.  One kernel on the current stream, no host
        synchronisation."""
        if not (origins.is_cuda and directions.is_cuda):
            raise RuntimeError(NO_CPU)
        if math.isnan(float(t_min)) or math.isnan(float(t_max)):
            raise ValueError(f"t_min and t_max must not be NaN, got {t_min}, {t_max}")
        G, dev = self.groups, self.vertices.device
        if origins.shape != directions.shape or origins.dim() not in (2, 3) or origins.size(-1) != 3:          # (the two as a pair)
            raise ValueError(f"origins and directions must both be (G, N, 3) or (N, 3), got {list(origins.shape)} / {list(directions.shape)}")
        origins, directions = self._group_points(origins, "rays"), self._group_points(directions, "rays")
        N = origins.size(1)
        hits = RayHits(torch.empty((G, N), dtype=torch.float32, device=dev), torch.empty((G, N), dtype=torch.int32, device=dev),
                       torch.empty((G, N, 2), dtype=torch.float32, device=dev) if barycentric else None)
        if N > 0:
            with torch.cuda.device(dev):
                s = raycast_struct(*self._description(), references=self._references, origins=origins, directions=directions,
                                   t=hits.t, triangle=hits.triangle, barycentric=hits.barycentric, t_min=t_min, t_max=t_max,
                                   cull_back=cull_back)
                _lib.check(_lib.load().pr_raycast_query(C.byref(s), torch.cuda.current_stream(dev).cuda_stream), "pr_raycast_query")
        if nearest:
            hits.nearest_t, hits.group = _nearest_group(hits.t, hits.triangle)
        return hits

    def closest(self, points: torch.Tensor, *, max_distance: float, point: bool = False, barycentric: bool = False,
                nearest: bool = False) -> "ClosestPoints":
        """The closest point of the meshes to every point, within ``max_distance``: ``points`` is ``(G, N, 3)`` - group g's points
        meet group g's mesh - or ``(N, 3)``, used for every group; in the meshes' frame.  ``max_distance`` has no default: the caller
        decides how far is too far to matter.  ``math.inf`` is allowed, but a point r cells from the mesh then visits the
        ``(2 r + 1)^3`` cells around it before it may stop, and its whole wave waits for it - a finite radius ends the search at that
        radius.  ``point`` / ``barycentric``: also the closest point itself and its ``(v, w)``.  ``nearest``: also the smallest
        distance over the groups and the group it belongs to.  The results are those of the exhaustive search over all triangles,
        bit for bit.  One kernel on the current stream, no host synchronisation."""
        if not points.is_cuda:
            raise RuntimeError(NO_CPU)
        if math.isnan(float(max_distance)) or float(max_distance) < 0:
            raise ValueError(f"max_distance must be >= 0 and not NaN, got {max_distance}")
        G, dev = self.groups, self.vertices.device
        points = self._group_points(points)
        N = points.size(1)
        found = ClosestPoints(torch.empty((G, N), dtype=torch.float32, device=dev), torch.empty((G, N), dtype=torch.int32, device=dev),
                              torch.empty((G, N, 3), dtype=torch.float32, device=dev) if point else None,
                              torch.empty((G, N, 2), dtype=torch.float32, device=dev) if barycentric else None)
        if N > 0:
            with torch.cuda.device(dev):
                s = closest_struct(*self._description(), references=self._references, points=points, distance=found.distance,
                                   triangle=found.triangle, point=found.point, barycentric=found.barycentric, max_distance=max_distance)
                _lib.check(_lib.load().pr_closest_query(C.byref(s), torch.cuda.current_stream(dev).cuda_stream), "pr_closest_query")
        if nearest:
            found.nearest_distance, found.group = _nearest_group(found.distance, found.triangle)
        return found

    def winding(self, points: torch.Tensor, *, axis: int = 2, crossings: bool = False) -> "Winding":
        """The winding number of the meshes around every point, along the coordinate axis ``axis`` (``pr_inside_query``): the
        signed count of the triangles that the ray from the point in the ``+axis`` direction passes through, +1 inside a closed mesh
        of the mesher's orientation.  ``points`` is ``(G, N, 3)`` or ``(N, 3)`` as for ``closest``.  ``crossings``: also the unsigned
        count.  Watertight by construction - the decisions the topology depends on are exact -, and equal to the exhaustive sum over
        all triangles whatever the grid.  The answer is a statement about a solid only for a mesh whose directed edges pair up: a
        mesh extracted with ``close_border=True`` (an uncapped mesh is open where it reaches the lattice border), simplified - if at
        all - with ``keep_duplicates=True``; ``RayGrid.audit`` says whether the mesh in hand is one (``balanced``).  For a point on the
        surface itself the three axes may differ.  One kernel on the current stream, no host synchronisation."""
        if not points.is_cuda:
            raise RuntimeError(NO_CPU)
        G, dev = self.groups, self.vertices.device
        points = self._group_points(points)
        try:
            axis = operator.index(axis)
        except TypeError:
            raise ValueError(f"axis must be 0, 1 or 2, got {axis!r}") from None
        if axis not in (0, 1, 2):
            raise ValueError(f"axis must be 0, 1 or 2, got {axis}")
        N = points.size(1)
        found = Winding(torch.empty((G, N), dtype=torch.int32, device=dev),
                        torch.empty((G, N), dtype=torch.int32, device=dev) if crossings else None)
        if N > 0:
            with torch.cuda.device(dev):
                s = inside_struct(*self._description(), references=self._references, points=points, axis=axis, winding=found.winding,
                                  crossings=found.crossings)
                _lib.check(_lib.load().pr_inside_query(C.byref(s), torch.cuda.current_stream(dev).cuda_stream), "pr_inside_query")
        return found

    def contains(self, points: torch.Tensor, *, axis: int = 2, any: bool = False):
        """Whether every point lies inside its group's mesh: bool ``(G, N)``, ``winding != 0``.  With ``any=True`` a triple: that,
        bool ``(N)`` - inside any group's mesh - and int64 ``(N)``, the lowest containing group or -1.  Meaningful for the meshes
        ``winding`` is meaningful for (capped with ``close_border=True``, duplicates kept when simplified); a point on the surface
        may fall on either side.  ``RayGrid.audit`` checks the mesh in hand (``balanced``).  A welded mesh (``weld_meshes``) answers
        identically.  No host synchronisation."""
        inside = self.winding(points, axis=axis).winding != 0
        if not any:
            return inside
        anywhere = inside.any(dim=0)
        lowest = torch.argmax(inside.to(torch.uint8), dim=0)             # (the first maximum: the lowest group that contains the point)
        return inside, anywhere, torch.where(anywhere, lowest, torch.full_like(lowest, -1))

    def signed_distance(self, points: torch.Tensor, *, max_distance: float, axis: int = 2, nearest: bool = False) -> torch.Tensor:
        """``closest``'s distance ``(G, N)``, negative where ``contains``; beyond ``max_distance`` it is ``-inf`` inside and ``+inf``
        outside.  ``nearest=True``: the minimum over the groups, ``(N)`` - the signed distance of the union of the solids.  Two
        launches (``pr_closest_query``, ``pr_inside_query``), no host synchronisation.  The sign is that of ``contains``: meaningful
        for capped meshes (``close_border=True``) that kept their duplicates when simplified (``keep_duplicates=True``).
        ``RayGrid.audit`` checks the mesh in hand (``balanced``)."""
        distance = self.closest(points, max_distance=max_distance).distance
        signed = torch.where(self.contains(points, axis=axis), -distance, distance)
        return signed.amin(dim=0) if nearest else signed

    def intersect(self, meshes: Optional[Sequence[Mesh]] = None, *, transform=None, pairs: bool = False, segments: bool = False,
                  self_: bool = False) -> List["MeshContacts"]:
        """The triangles of ``meshes`` - one per group, posed by ``transform`` (``v' = R v + t``: one ``(3, 4)`` / ``(4, 4)`` matrix for
        all groups, or ``(G, 3, 4)`` / ``(G, 4, 4)``; None: as they are) - that cut the triangles of this grid's meshes
        (``pr_mesh_intersect``): one ``MeshContacts`` per group.  Two triangles are a pair iff their boxes overlap and an edge of one
        passes through the other, decided in fixed fp32 arithmetic with a conditioning clause - coplanar overlap is never a pair, and the
        result is that of the exhaustive rule over all pairs, bit for bit, whatever the grid.  ``self_=True``: the grid's meshes
        against themselves (``meshes`` and ``transform`` must be None) - pairs of one triangle with itself and of triangles that share
        a corner value are left out, and every unordered pair shows up twice.  Without ``pairs`` / ``segments`` one counting call and no
        host synchronisation; with them the number of pairs is read back - the ONE synchronisation -, an exactly sized emitting call
        follows, and one sort puts the pairs into (query, target) order.  A static object's grid is built once and the moving object
        posed per call: cheaper than ``Mesh.transformed`` and a rebuild."""
        G, dev = self.groups, self.vertices.device
        if not self.vertices.is_cuda:
            raise RuntimeError(NO_CPU)
        if self_:
            if meshes is not None or transform is not None:
                raise ValueError("self_=True queries the grid's own meshes: meshes and transform must be None")
            to = self._triangle_bounds()
            query = {}
            QT = self.total_triangles
        else:
            meshes = list(meshes) if meshes is not None else []
            if len(meshes) != G:
                raise ValueError(f"the grid holds {G} groups, got {len(meshes)} meshes")
            _device_of(meshes)
            q = _pack_meshes(meshes, dev)                              # (on the grid's device)
            to, QT = q.to, q.T
            names = ("q_vertices", "q_triangles", "q_vertex_offsets", "q_triangle_offsets", "q_total_vertices", "q_total_triangles")
            query = dict(zip(names, q.arguments()), transform=_pose_rows(transform, G, dev))
        count = torch.empty(max(QT, 1), dtype=torch.int32, device=dev)
        first = torch.empty(max(QT, 1), dtype=torch.int32, device=dev)
        offsets = torch.empty(QT + 1, dtype=torch.int32, device=dev)
        pair_rows = segment_rows = None
        bounds = [0] * (G + 1)
        with torch.cuda.device(dev):
            common = self._description()
            outputs = dict(references=self._references, count=count, first=first, pair_offsets=offsets, self_=self_, **query)
            workspace, size = _call_with_workspace("pr_mesh_intersect_workspace_size", "pr_mesh_intersect",
                                                   intersect_struct(*common, **outputs), dev)
            if pairs or segments:
                bounds = offsets[torch.tensor(to, dtype=torch.int64, device=dev)].cpu().tolist()          # (the host synchronisation)
                P = bounds[-1]
                if P < 0:
                    raise RuntimeError("2^31 or more pairs")
                pair_rows = torch.empty((P, 2), dtype=torch.int32, device=dev)
                segment_rows = torch.empty((P, 2, 3), dtype=torch.float32, device=dev) if segments else None
                if P > 0:
                    _call("pr_mesh_intersect", intersect_struct(*common, pairs=pair_rows, segments=segment_rows, **outputs), workspace, size, dev)
                    # (packed query row, target) as one key: the rows of a query are already adjacent, the sort orders them inside
                    row = torch.repeat_interleave(torch.arange(QT, dtype=torch.int64, device=dev), count[:QT].to(torch.int64), output_size=P)
                    order = torch.sort(row * (self.total_triangles + 1) + pair_rows[:, 1].to(torch.int64)).indices
                    pair_rows = pair_rows[order]
                    segment_rows = segment_rows[order] if segments else None
        out = []
        for g in range(G):
            own = offsets[to[g]:to[g + 1] + 1]
            out.append(MeshContacts(count[to[g]:to[g + 1]], first[to[g]:to[g + 1]], own - own[:1],
                                    pair_rows[bounds[g]:bounds[g + 1]] if pair_rows is not None else None,
                                    segment_rows[bounds[g]:bounds[g + 1]] if segment_rows is not None else None, symmetric=bool(self_)))
        return out


@dataclass
class Winding:
    """What ``RayGrid.winding`` returns: ``winding (G, N)`` int32 and ``crossings (G, N)`` int32 - how many triangles the ray from
    the point passes through - or None."""
    winding: torch.Tensor
    crossings: Optional[torch.Tensor] = None


def inside_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                  total_vertices: int, total_triangles: int, origin, cell, cells, cell_offsets: torch.Tensor, *,
                  references: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None, axis: int = 2,
                  winding: Optional[torch.Tensor] = None, crossings: Optional[torch.Tensor] = None) -> _lib.Inside:
    """``pr_inside_t`` over prepared tensors (fp32 / int32, contiguous, one device); ``max_references`` is the rows of ``references``,
    ``count`` the second dimension of ``points (G, N, 3)``."""
    s = _lib.Inside()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles)
    _set_grid(s, origin, cell, cells)
    s.max_references = 0 if references is None else references.size(0)
    s.count = 0 if points is None else points.size(1)
    s.axis = int(axis)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         cell_offsets=cell_offsets, references=references, points=points, winding=winding, crossings=crossings)


def closest_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                   total_vertices: int, total_triangles: int, origin, cell, cells, cell_offsets: torch.Tensor, *,
                   references: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None,
                   distance: Optional[torch.Tensor] = None, triangle: Optional[torch.Tensor] = None,
                   point: Optional[torch.Tensor] = None, barycentric: Optional[torch.Tensor] = None,
                   max_distance: float = math.inf) -> _lib.Closest:
    """``pr_closest_t`` over prepared tensors (fp32 / int32, contiguous, one device); ``max_references`` is the rows of ``references``,
    ``count`` the second dimension of ``points (G, N, 3)``."""
    s = _lib.Closest()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles)
    _set_grid(s, origin, cell, cells)
    s.max_references = 0 if references is None else references.size(0)
    s.count = 0 if points is None else points.size(1)
    s.max_distance = float(max_distance)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         cell_offsets=cell_offsets, references=references, points=points, distance=distance, triangle=triangle,
                         point=point, barycentric=barycentric)


@dataclass
class ClosestPoints:
    """What ``RayGrid.closest`` returns: ``distance (G, N)`` (``+inf``: nothing within ``max_distance``), ``triangle (G, N)`` int32 local
    to the group (-1: a miss), ``point (G, N, 3)`` - the closest point, zeros for a miss - or None, ``barycentric (G, N, 2)`` =
    ``(v, w)`` (the point is ``a + v (b - a) + w (c - a)``) or None; with ``nearest=True`` also ``nearest_distance (N)`` and ``group
    (N)`` int64: the smallest distance over the groups and the group it belongs to (-1: none found)."""
    distance: torch.Tensor
    triangle: torch.Tensor
    point: Optional[torch.Tensor] = None
    barycentric: Optional[torch.Tensor] = None
    nearest_distance: Optional[torch.Tensor] = None
    group: Optional[torch.Tensor] = None


AUDIT_COUNT_FIELDS = ("candidates", "dropped", "vertices", "edges", "unbalanced_edges", "boundary_edges", "non_manifold_edges",
                      "euler_characteristic", "shells", "largest_shell")


@dataclass
class MeshAudit:
    """What ``audit_meshes`` returns per mesh, on the device: ``counts (12)`` int32 and ``measures (8)`` fp64 as ``pr_mesh_audit``
    (include/playrender.h) defines them, and ``labels (T)`` int32 - per triangle the lowest triangle index of its shell, -1 for a
    dropped triangle - or None.  ``report()`` reads them back."""
    counts: torch.Tensor
    measures: torch.Tensor
    labels: Optional[torch.Tensor] = None

    def report(self) -> dict:
        """The audit as a plain dict - ONE read-back: the ten counts by name (``AUDIT_COUNT_FIELDS``), ``area``, ``signed_volume``,
        ``centroid`` (three floats), ``balanced`` - every directed edge, by vertex value, occurs as often as its reverse: what
        ``RayGrid.contains`` needs - and ``closed_manifold`` - also no boundary and no non-manifold edge."""
        host = torch.cat([self.counts.reshape(-1).to(torch.float64), self.measures.reshape(-1).to(torch.float64)]).cpu().tolist()      # (int32 is exact in fp64)
        out = {name: int(host[i]) for i, name in enumerate(AUDIT_COUNT_FIELDS)}
        m = host[_lib.AUDIT_COUNTS:]
        out["area"], out["signed_volume"], out["centroid"] = m[0], m[1], m[2:5]
        out["balanced"] = out["unbalanced_edges"] == 0
        out["closed_manifold"] = out["balanced"] and out["boundary_edges"] == 0 and out["non_manifold_edges"] == 0
        return out


def audit_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                 total_vertices: int, total_triangles: int, counts: torch.Tensor, *, measures: Optional[torch.Tensor] = None,
                 labels: Optional[torch.Tensor] = None) -> _lib.MeshAudit:
    """``pr_mesh_audit_t`` over prepared tensors (fp32 / int32 / fp64, contiguous, one device)."""
    s = _lib.MeshAudit()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         counts=counts, measures=measures, labels=labels)


def _audit_packed(vertices, triangles, vertex_offsets, triangle_offsets, V: int, T: int, labels: bool):
    """One ``pr_mesh_audit`` call on packed device tensors (``_PackedMeshes.arguments`` or a grid's), on the current stream:
    ``(counts (G, 12), measures (G, 8), labels (T) or None)``.  The workspace is sized on the host; nothing is read back."""
    dev = vertices.device
    G = vertex_offsets.numel() - 1
    with torch.cuda.device(dev):
        counts = torch.empty((G, _lib.AUDIT_COUNTS), dtype=torch.int32, device=dev)
        measures = torch.empty((G, _lib.AUDIT_MEASURES), dtype=torch.float64, device=dev)
        shell = torch.empty(T, dtype=torch.int32, device=dev) if labels else None
        s = audit_struct(vertices, triangles, vertex_offsets, triangle_offsets, V, T, counts, measures=measures,
                         labels=shell if labels and T > 0 else None)         # (no triangles: an empty ``shell`` is returned, NULL is passed)
        _call_with_workspace("pr_mesh_audit_workspace_size", "pr_mesh_audit", s, dev)
    return counts, measures, shell


def audit_meshes(meshes: Sequence[Mesh], *, labels: bool = False) -> List[MeshAudit]:
    """How the meshes are made up (``pr_mesh_audit``, include/playrender.h), one ``MeshAudit`` per mesh.  Vertices are identified by
    VALUE, as ``RayGrid.contains`` sees them, so the coinciding vertices the mesher emits for lattice values equal to the level do
    not make a mesh look open.  ``counts``: candidate and dropped triangles, distinct referenced vertices, undirected edges,
    unbalanced / boundary / non-manifold edges, Euler characteristic, shells, triangles of the largest shell.  ``measures``: area,
    signed volume (positive for the mesher's orientation), area-weighted centroid - float64 sums in a fixed tree, equal from run to
    run.  ``labels=True``: also the shell of every triangle (``Mesh.keep_shells`` uses them).

    The meshes are packed (``_pack_meshes``); the workspace is sized on the host; one call on the current stream
    and NO host synchronisation - ``MeshAudit.report()`` is the read-back.  There is no CPU fallback."""
    meshes = _listed(meshes, "audit_meshes")
    p = _pack_meshes(meshes, _device_of(meshes))
    counts, measures, shell = _audit_packed(*p.arguments(), bool(labels))
    return [MeshAudit(counts[g], measures[g], shell[p.to[g]:p.to[g + 1]] if labels else None) for g in range(p.groups)]


def weld_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                total_vertices: int, total_triangles: int, counts: torch.Tensor, out_vertex_offsets: torch.Tensor,
                out_triangle_offsets: torch.Tensor, *, normals: Optional[torch.Tensor] = None,
                attributes: Optional[torch.Tensor] = None, out_vertices: Optional[torch.Tensor] = None,
                out_normals: Optional[torch.Tensor] = None, out_attributes: Optional[torch.Tensor] = None,
                out_triangles: Optional[torch.Tensor] = None, vertex_map: Optional[torch.Tensor] = None,
                triangle_map: Optional[torch.Tensor] = None, merge: bool = True) -> _lib.MeshWeld:
    """``pr_mesh_weld_t`` over prepared tensors (fp32 / int32, contiguous, one device); the capacities are the outputs' rows and the
    attribute width is the second dimension of ``attributes``."""
    s = _lib.MeshWeld()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, 0 if merge else _lib.WELD_COMPACT_ONLY)
    s.attribute_width = 0 if attributes is None else attributes.size(1)
    s.max_vertices = 0 if out_vertices is None else out_vertices.size(0)
    s.max_triangles = 0 if out_triangles is None else out_triangles.size(0)
    return _set_pointers(s, vertices=vertices, normals=normals, attributes=attributes, triangles=triangles,
                         vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets, out_vertices=out_vertices,
                         out_normals=out_normals, out_attributes=out_attributes, out_triangles=out_triangles, vertex_map=vertex_map,
                         triangle_map=triangle_map, counts=counts, out_vertex_offsets=out_vertex_offsets,
                         out_triangle_offsets=out_triangle_offsets)


def _weld_packed(p: _PackedMeshes, merge: bool, maps: bool):
    """``pr_mesh_weld`` on packed meshes, on ``_simplify_packed``'s route: a counting call, one read-back of the two offset arrays,
    an exactly sized emitting call.  Returns ``(meshes, vertex_maps, triangle_maps)``; the maps are None without ``maps``."""
    dev, G, V, T = p.vertices.device, p.groups, p.V, p.T
    inputs = dict(normals=p.normals, attributes=p.attributes, merge=merge)
    with torch.cuda.device(dev):
        offsets = torch.empty((2, G + 1), dtype=torch.int32, device=dev)
        counts = torch.empty((G, _lib.WELD_COUNTS), dtype=torch.int32, device=dev)
        common = (*p.arguments(), counts, offsets[0], offsets[1])
        workspace, size = _call_with_workspace("pr_mesh_weld_workspace_size", "pr_mesh_weld", weld_struct(*common, **inputs), dev)
        out_vo, out_to = offsets.cpu().tolist()                             # (the host synchronisation)
        out_v = torch.empty((out_vo[G], 3), dtype=torch.float32, device=dev)
        out_n = None if p.normals is None else torch.empty((out_vo[G], 3), dtype=torch.float32, device=dev)
        out_a = None if p.attributes is None else torch.empty((out_vo[G], p.attributes.size(1)), dtype=torch.float32, device=dev)
        out_t = torch.empty((out_to[G], 3), dtype=torch.int32, device=dev)
        vmap = torch.full((V,), -1, dtype=torch.int32, device=dev) if maps else None
        tmap = torch.full((T,), -1, dtype=torch.int32, device=dev) if maps else None
        if out_vo[G] > 0 or (maps and V + T > 0):
            some = out_vo[G] > 0                                    # (a kept triangle refers to three output vertices)
            emit = weld_struct(*common, **inputs, out_vertices=out_v if some else None, out_normals=out_n if some else None,
                               out_attributes=out_a if some else None, out_triangles=out_t if some else None,
                               vertex_map=vmap if maps and V > 0 else None, triangle_map=tmap if maps and T > 0 else None)
            _call("pr_mesh_weld", emit, workspace, size, dev)
    meshes = [Mesh(out_v[out_vo[g]:out_vo[g + 1]], out_t[out_to[g]:out_to[g + 1]], None if out_n is None else out_n[out_vo[g]:out_vo[g + 1]],
                   None if out_a is None else out_a[out_vo[g]:out_vo[g + 1]]) for g in range(G)]
    if not maps:
        return meshes, None, None
    return meshes, [vmap[p.vo[g]:p.vo[g + 1]] for g in range(G)], [tmap[p.to[g]:p.to[g + 1]] for g in range(G)]


def weld_meshes(meshes: Sequence[Mesh], *, merge: bool = True, maps: bool = False):
    """The meshes welded and compacted (``pr_mesh_weld``, include/playrender.h): vertices of a mesh whose three components compare
    equal become ONE vertex - the one with the lowest index, whose position, normal and feature rows are copied bit for bit; nothing
    is averaged -, vertices that no kept triangle refers to go, and so do the triangles that ``audit_meshes`` counts as dropped (an
    index out of range, a vertex that is not finite, ``a == b`` or ``a == c`` as values).  The kept triangles keep their order and
    orientation.  In the result identity by index IS identity by value: what an OBJ viewer or an adjacency builder needs, while
    ``RayGrid.contains`` and ``audit_meshes`` answer as on the input.  ``merge=False`` merges nothing and only drops the dead rows.

    The meshes are packed (``_pack_meshes``), counted, and - after reading the two offset arrays back, the ONE host
    synchronisation - emitted into exactly sized tensors.  Returns one mesh per input; they have normals iff every input has them,
    and ``features`` iff every input has them with one common width - carried as fp32 attribute rows, so the result's features
    are fp32 whatever the input's dtype.  ``maps=True``: a triple ``(meshes, vertex_maps, triangle_maps)`` of lists, per mesh int32
    ``(V)`` - the output index of every input vertex's representative, -1 if it is not finite or unreferenced - and int32 ``(T)`` -
    the output index of every kept triangle, -1 for a dropped one.  There is no CPU fallback."""
    meshes = _listed(meshes, "weld_meshes")
    dev = _device_of(meshes)
    _mesh_shapes(meshes)                                            # (refused before the features' width, which the packer needs)
    width = _feature_width(meshes, _lib.WELD_MAX_ATTRIBUTE_WIDTH)   # (0: the rows are still counted, nothing is carried)
    p = _pack_meshes(meshes, dev, normals=all(m.normals is not None for m in meshes), features=width)
    out, vmaps, tmaps = _weld_packed(p, bool(merge), bool(maps))
    return (out, vmaps, tmaps) if maps else out


def smooth_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                  total_vertices: int, total_triangles: int, out_vertices: torch.Tensor, counts: torch.Tensor, *, steps: int = 0,
                  lam: float = 0.5, mu: float = -0.53, max_degree: int = 64, pin_border: bool = True,
                  pinned: Optional[torch.Tensor] = None, out_normals: Optional[torch.Tensor] = None,
                  incidence_offsets: Optional[torch.Tensor] = None, incidence: Optional[torch.Tensor] = None,
                  vertex_state: Optional[torch.Tensor] = None) -> _lib.MeshSmooth:
    """``pr_mesh_smooth_t`` over prepared tensors (fp32 / int32 / uint8, contiguous, one device)."""
    s = _lib.MeshSmooth()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, _lib.SMOOTH_PIN_BORDER if pin_border else 0)
    s.steps = int(steps)
    s.max_degree = int(max_degree)
    s.lambda_ = float(lam)
    s.mu = float(mu)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         pinned=pinned, out_vertices=out_vertices, out_normals=out_normals, incidence_offsets=incidence_offsets,
                         incidence=incidence, vertex_state=vertex_state, counts=counts)


def _smooth_packed(p: _PackedMeshes, *, steps, lam, mu, max_degree, pin_border, pinned=None, normals=True, incidence=False, state=False):
    """``pr_mesh_smooth`` on packed meshes: ONE call into exactly sized tensors - the sizes do not change - and no host
    synchronisation.  Returns a dict of the packed outputs."""
    dev, G, V, T = p.vertices.device, p.groups, p.V, p.T
    row = lambda n: max(n, 1)            # (outputs the library wants an address for: one row at least, sliced back to V below)
    with torch.cuda.device(dev):
        mesh = p.arguments()
        out = {"vertices": torch.empty((row(V), 3), dtype=torch.float32, device=dev),
               "counts": torch.empty((G, _lib.SMOOTH_COUNTS), dtype=torch.int32, device=dev)}
        if normals:
            out["normals"] = torch.empty((row(V), 3), dtype=torch.float32, device=dev)
        if incidence:
            out["incidence_offsets"] = torch.empty(V + 1, dtype=torch.int32, device=dev)
            out["incidence"] = torch.empty(row(3 * T), dtype=torch.int32, device=dev)
        if state:
            out["state"] = torch.empty(row(V), dtype=torch.int32, device=dev)
        if pinned is not None and pinned.numel() == 0:
            pinned = None                                             # (an optional input: NULL, not a placeholder)
        s = smooth_struct(*mesh, out["vertices"], out["counts"], steps=steps, lam=lam, mu=mu, max_degree=max_degree,
                          pin_border=pin_border, pinned=pinned, out_normals=out.get("normals"),
                          incidence_offsets=out.get("incidence_offsets"), incidence=out.get("incidence"), vertex_state=out.get("state"))
        _call_with_workspace("pr_mesh_smooth_workspace_size", "pr_mesh_smooth", s, dev)
    for key in ("vertices", "normals", "state"):
        if key in out:
            out[key] = out[key][:V]
    return out


def _smooth_arguments(iterations, lam, mu, max_degree):
    """``(steps, lam, mu, max_degree)`` checked as ``pr_mesh_smooth`` checks them, with the argument's own name in the message."""
    try:
        iterations, max_degree = operator.index(iterations), operator.index(max_degree)
    except TypeError:
        raise ValueError(f"iterations and max_degree must be integers, got {iterations!r} / {max_degree!r}") from None
    steps = iterations if mu is None else 2 * iterations
    if iterations < 0 or steps > _lib.SMOOTH_MAX_STEPS:
        raise ValueError(f"iterations must give 0 .. {_lib.SMOOTH_MAX_STEPS} steps (two per iteration with mu), got {iterations}")
    if not 1 <= max_degree <= _lib.SMOOTH_MAX_DEGREE:
        raise ValueError(f"max_degree must be 1 .. {_lib.SMOOTH_MAX_DEGREE}, got {max_degree}")
    lam = float(lam)
    mu = lam if mu is None else float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"lam and mu must be finite, got {lam} / {mu}")
    return steps, lam, mu, max_degree


def smooth_meshes(meshes: Sequence[Mesh], *, iterations: int = 10, lam: float = 0.5, mu: Optional[float] = -0.53,
                  pin_border: bool = True, pinned=None, weld: bool = True, normals: bool = True, max_degree: int = 64,
                  report: bool = False):
    """The meshes smoothed (``pr_mesh_smooth``, include/playrender.h): ``iterations`` Taubin iterations - a step with the factor
    ``lam``, then one with ``mu`` (``mu < -lam < 0`` keeps the volume), ``steps = 2 * iterations`` - of the triangle umbrella on the
    vertex-to-triangle incidence lists, deterministic bit for bit.  ``mu=None``: plain Laplacian smoothing, ``steps = iterations`` with
    ``lam`` alone (the mesh shrinks).  Triangles are untouched, so the topology - and with it ``audit_meshes``' counts - stays.

    Identity is by INDEX: with ``weld=True`` (the default) the meshes go through ``weld_meshes`` first - its read-back is the ONE host
    synchronisation; ``weld=False`` is for meshes that are welded already and synchronises nothing (an unwelded mesh tears at its
    coinciding vertices).  ``pin_border``: vertices on an open border stay.  ``pinned``: per mesh a ``(V)`` mask (or None) of vertices
    that stay - rows of the mesh as smoothed, so with ``weld=True`` of the WELDED mesh.  Vertices with more than ``max_degree``
    (1 .. 256) incident triangles stay and get a zero normal.  ``normals=True`` replaces the normals by the area-weighted normals of
    the smoothed triangles (zero rows where a vertex has no valid triangle); at False the input's normals are carried.  Features
    are carried row for row (vertex counts do not change after the weld).  Returns one mesh per input; ``report=True``: a triple
    ``(meshes, counts, states)`` of lists with the ``(8)`` counts and the ``(V)`` state words of every mesh (header), still on the
    device.  There is no CPU fallback."""
    meshes = _listed(meshes, "smooth_meshes")
    dev = _device_of(meshes)
    steps, lam, mu, max_degree = _smooth_arguments(iterations, lam, mu, max_degree)
    if weld:
        meshes = weld_meshes(meshes)                                  # (its first refusal is the packer's: the shapes)
    packed = _pack_meshes(meshes, dev)
    mask = None
    if pinned is not None:
        pinned = list(pinned)
        if len(pinned) != len(meshes):
            raise ValueError(f"pinned must hold one mask (or None) per mesh, got {len(pinned)} for {len(meshes)} meshes")
        parts = []
        for m, p in zip(meshes, pinned):
            if p is None:
                parts.append(torch.zeros(m.vertices.size(0), dtype=torch.uint8, device=dev))
                continue
            if p.numel() != m.vertices.size(0):
                raise ValueError(f"a pinned mask must have one entry per vertex of the mesh as it is smoothed ({m.vertices.size(0)}), "
                                 f"got {p.numel()}")
            parts.append((p.detach().to(dev).reshape(-1) != 0).to(torch.uint8))
        mask = torch.cat(parts).contiguous()
    out = _smooth_packed(packed, steps=steps, lam=lam, mu=mu, max_degree=max_degree, pin_border=bool(pin_border), pinned=mask,
                         normals=bool(normals), state=bool(report))
    result = []
    for g, m in enumerate(meshes):
        v0, v1 = packed.vo[g], packed.vo[g + 1]
        result.append(Mesh(out["vertices"][v0:v1], m.triangles, out["normals"][v0:v1] if normals else m.normals, m.features))
    if not report:
        return result
    return result, [out["counts"][g] for g in range(packed.groups)], [out["state"][packed.vo[g]:packed.vo[g + 1]] for g in range(packed.groups)]


def sample_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                  total_vertices: int, total_triangles: int, samples: int, seed: int, points: torch.Tensor, counts: torch.Tensor,
                  measures: torch.Tensor, *, first: int = 0, face_normals: bool = False, normals: Optional[torch.Tensor] = None,
                  attributes: Optional[torch.Tensor] = None, triangle: Optional[torch.Tensor] = None,
                  barycentric: Optional[torch.Tensor] = None, out_normals: Optional[torch.Tensor] = None,
                  out_attributes: Optional[torch.Tensor] = None) -> _lib.MeshSample:
    """``pr_mesh_sample_t`` over prepared tensors (fp32 / int32 / fp64, contiguous, one device); the attribute width is the second
    dimension of ``attributes``."""
    s = _lib.MeshSample()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, _lib.SAMPLE_FACE_NORMALS if face_normals else 0)
    s.samples = int(samples)
    s.attribute_width = 0 if attributes is None else attributes.size(1)
    s.seed = int(seed)
    s.first_sample = int(first)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         normals=normals, attributes=attributes, points=points, triangle=triangle, barycentric=barycentric,
                         out_normals=out_normals, out_attributes=out_attributes, counts=counts, measures=measures)


@dataclass
class SurfaceSamples:
    """What ``sample_meshes`` returns per mesh, on the device: ``points (n, 3)``, ``triangle (n)`` int32 - the triangle every point lies
    on, -1 throughout for a mesh without area -, ``barycentric (n, 2)`` = ``(v, w)`` of the point in it (``RayGrid.closest``'s
    convention: the point is ``a + v (b - a) + w (c - a)``), ``normals (n, 3)`` unit vectors (zero rows where there is none) or None,
    ``features (n, F)`` fp32 or None, ``counts (4)`` int32 - valid triangles, dropped triangles, valid triangles too small to be drawn,
    points drawn - and ``measures (2)`` fp64: the largest triangle area and the area the points are spread over."""
    points: torch.Tensor
    triangle: torch.Tensor
    barycentric: torch.Tensor
    normals: Optional[torch.Tensor]
    features: Optional[torch.Tensor]
    counts: torch.Tensor
    measures: torch.Tensor


def _sample_arguments(n, seed, first, groups):
    """``(n, seed, first)`` checked as ``pr_mesh_sample`` checks them, with the argument's own name in the message."""
    try:
        n, seed, first = operator.index(n), operator.index(seed), operator.index(first)
    except TypeError:
        raise ValueError(f"n, seed and first must be integers, got {n!r} / {seed!r} / {first!r}") from None
    if n < 0 or groups * n >= 2 ** 31:
        raise ValueError(f"n must be >= 0 with meshes * n below 2^31, got {n} for {groups} meshes")
    if not (0 <= seed < 2 ** 64 and 0 <= first < 2 ** 64):
        raise ValueError(f"seed and first must be in [0, 2^64), got {seed} / {first}")
    return n, seed, first


def _sample_packed(vertices, triangles, vertex_offsets, triangle_offsets, V: int, T: int, n: int, seed: int, first: int, *,
                   face: bool = False, normals=None, attributes=None):
    """One ``pr_mesh_sample`` call on packed device tensors (the offsets too), on the current stream, into exactly sized tensors:
    a dict of the ``(G, n, ...)`` outputs.  The workspace is sized on the host; nothing is read back."""
    dev = vertices.device
    G = vertex_offsets.numel() - 1
    rows = max(G * n, 1)                                            # (outputs the library wants an address for; sliced back below)
    with torch.cuda.device(dev):
        new = lambda width, dtype=torch.float32: torch.empty((rows, width), dtype=dtype, device=dev)
        out = {"points": new(3), "triangle": new(1, torch.int32), "barycentric": new(2),
               "counts": torch.empty((G, _lib.SAMPLE_COUNTS), dtype=torch.int32, device=dev),
               "measures": torch.empty((G, _lib.SAMPLE_MEASURES), dtype=torch.float64, device=dev)}
        if face or normals is not None:
            out["normals"] = new(3)
        if attributes is not None:
            out["features"] = new(attributes.size(1))
        s = sample_struct(vertices, triangles, vertex_offsets, triangle_offsets, V, T, n, seed, out["points"], out["counts"],
                          out["measures"], first=first, face_normals=face, normals=None if face else normals, attributes=attributes,
                          triangle=out["triangle"], barycentric=out["barycentric"], out_normals=out.get("normals"),
                          out_attributes=out.get("features"))
        _call_with_workspace("pr_mesh_sample_workspace_size", "pr_mesh_sample", s, dev)
    for key in ("points", "triangle", "barycentric", "normals", "features"):
        if key in out:
            out[key] = out[key][:G * n].reshape((G, n) + ((out[key].size(1),) if key != "triangle" else ()))
    return out


def _surface_samples(out, groups: int) -> List[SurfaceSamples]:
    pick = lambda key, g: out[key][g] if key in out else None
    return [SurfaceSamples(out["points"][g], out["triangle"][g], out["barycentric"][g], pick("normals", g), pick("features", g),
                           out["counts"][g], out["measures"][g]) for g in range(groups)]


def sample_meshes(meshes: Sequence[Mesh], n: int, *, seed: int, first: int = 0, normals: Optional[str] = "face",
                  features: bool = True) -> List[SurfaceSamples]:
    """``n`` points on every mesh, drawn with probability proportional to triangle area (``pr_mesh_sample``, include/playrender.h),
    one ``SurfaceSamples`` per mesh: the point cloud of an object, and what a surface integral over a mesh is made from
    (``compare_meshes``).  Point ``i`` of mesh ``g`` is a function of ``(seed, first + i, g)`` and of the mesh alone - Philox draws,
    integer weights and integer prefix sums -, so the result is equal bit for bit from run to run, points ``[k, n)`` are points
    ``[0, n - k)`` of the call with ``first + k``, and two calls whose ranges ``[first, first + n)`` do not meet draw independent
    points.  ``seed`` has no default: the caller owns repeatability.  Triangles with an index out of range, a repeated index or a
    coordinate that is not finite are not drawn from, nor are triangles below ``2^-32`` of the mesh's largest (``counts`` reports
    both); a mesh without area gets ``triangle == -1`` and zeros.

    ``normals``: ``"face"`` (the default) - the unit normal of the triangle the point lies on, pointing where the triangle points;
    ``"vertex"`` - the meshes' vertex normals interpolated to the point and normalised, which raises for a mesh without normals; None.
    ``features=True`` carries ``Mesh.features`` to the points where every mesh has them with one common width - as fp32 rows,
    whatever their dtype, as ``weld_meshes`` carries them.

    The meshes are packed (``_pack_meshes``); the workspace is sized on the host; one call on the current stream and
    NO host synchronisation.  There is no CPU fallback."""
    meshes = _listed(meshes, "sample_meshes")
    if normals not in ("vertex", "face", None):
        raise ValueError(f"normals must be 'vertex', 'face' or None, got {normals!r}")
    n, seed, first = _sample_arguments(n, seed, first, len(meshes))
    dev = _device_of(meshes)
    _mesh_shapes(meshes)                                            # (refused before the two below, which the packer needs)
    if normals == "vertex" and not all(m.normals is not None for m in meshes):
        raise ValueError("normals='vertex' needs meshes with normals (Mesh.vertex_normals() computes them); 'face' needs none")
    width = _feature_width(meshes, _lib.SAMPLE_MAX_ATTRIBUTE_WIDTH) if features else None
    p = _pack_meshes(meshes, dev, normals=normals == "vertex", features=width or None)     # (0: as without features)
    out = _sample_packed(*p.arguments(), n, seed, first, face=normals == "face", normals=p.normals, attributes=p.attributes)
    return _surface_samples(out, p.groups)


DEVIATION_FIELDS = ("samples", "misses", "mean", "rms", "max", "p99", "normal_consistency")


@dataclass
class MeshDeviation:
    """What ``compare_meshes`` returns, on the device: per direction a fp64 vector of ``DEVIATION_FIELDS`` followed by one share per
    threshold, the ``(samples)`` fp32 distances they were reduced from (``+inf``: a miss) and the thresholds.  ``report()`` reads
    them back."""
    a_to_b: torch.Tensor
    b_to_a: torch.Tensor
    distance_a_to_b: torch.Tensor
    distance_b_to_a: torch.Tensor
    thresholds: tuple = ()

    def report(self) -> dict:
        """The deviation as a plain dict - ONE read-back.  ``a_to_b`` / ``b_to_a``: ``samples``, ``misses`` - samples with nothing of
        the other mesh within ``max_distance``; they are left out of the means and always reported -, ``mean``, ``rms``, ``max``
        and ``p99`` (nearest rank) of the found distances (NaN if none was found), ``normal_consistency`` - the mean ``|n . n'|`` of
        the sample's face normal and the closest triangle's over the found samples where neither is zero - and ``within``: per
        threshold the share of ALL samples, misses included, within it.  ``chamfer = a_to_b.mean + b_to_a.mean``.  ``thresholds``:
        per threshold ``precision`` (the share of a within it of b), ``recall`` (of b within it of a) and ``fscore``, their harmonic
        mean (0 where both are 0)."""
        host = torch.stack([self.a_to_b, self.b_to_a]).cpu().tolist()
        k = len(DEVIATION_FIELDS)
        out = {}
        for name, row in zip(("a_to_b", "b_to_a"), host):
            side = dict(zip(DEVIATION_FIELDS, row))
            side["samples"], side["misses"] = int(side["samples"]), int(side["misses"])
            side["within"] = list(row[k:])
            out[name] = side
        out["chamfer"] = out["a_to_b"]["mean"] + out["b_to_a"]["mean"]
        out["thresholds"] = []
        for i, threshold in enumerate(self.thresholds):
            precision, recall = host[0][k + i], host[1][k + i]
            fscore = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
            out["thresholds"].append({"threshold": threshold, "precision": precision, "recall": recall, "fscore": fscore})
        return out


def _unit_rows(n: torch.Tensor) -> torch.Tensor:
    length = n.norm(dim=1, keepdim=True)
    return torch.where((length > 0) & torch.isfinite(length), n / length, torch.zeros_like(n))


def _one_sided_deviation(samples: SurfaceSamples, other: Mesh, grid: "RayGrid", max_distance: float, thresholds):
    """``(statistics, distances)`` of one direction: plain torch expressions in fp64, nothing is read back."""
    found = grid.closest(samples.points, max_distance=max_distance)
    distance, triangle = found.distance[0], found.triangle[0]
    d = distance.to(torch.float64)
    hit = torch.isfinite(d) & (triangle >= 0)
    total = torch.tensor(float(d.numel()), dtype=torch.float64, device=d.device)
    m = hit.sum()
    count = m.to(torch.float64)                                      # (0 found: 0 / 0 = NaN in the means)
    nan = torch.full_like(count, math.nan)
    zero = torch.zeros_like(d)
    mean = torch.where(hit, d, zero).sum() / count
    rms = torch.sqrt(torch.where(hit, d * d, zero).sum() / count)
    largest = torch.where(m > 0, torch.where(hit, d, torch.full_like(d, -math.inf)).max(), nan)
    # nearest rank: the smallest found distance that at least 99 % of the found distances do not exceed
    ordered = torch.sort(torch.where(hit, d, torch.full_like(d, math.inf))).values
    rank = ((99 * m + 99) // 100 - 1).clamp(min=0)
    p99 = torch.where(m > 0, ordered[rank], nan)
    # the closest triangle's face normal, in fp64, against the sample's
    face = torch.zeros((d.numel(), 3), dtype=torch.float64, device=d.device)
    if other.triangles.size(0) > 0:
        rows = triangle.clamp(min=0, max=other.triangles.size(0) - 1).to(torch.int64)
        corners = other.vertices.detach().to(torch.float64)[other.triangles.detach().to(torch.int64)[rows]]
        face = _unit_rows(torch.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], dim=1))
    own = _unit_rows(samples.normals.to(torch.float64))
    both = hit & (face != 0).any(dim=1) & (own != 0).any(dim=1)
    dots = (face * own).sum(dim=1).abs()
    consistency = torch.where(both, dots, zero).sum() / both.sum().to(torch.float64)
    shares = [(d <= t).sum().to(torch.float64) / total for t in thresholds]            # (a miss is +inf: within nothing)
    return torch.stack([total, total - count, mean, rms, largest, p99, consistency] + shares), distance


def compare_meshes(a: Mesh, b: Mesh, *, samples: int, seed: int, max_distance: float, thresholds=(), cells=32) -> MeshDeviation:
    """How far two meshes lie from each other, as surface integrals: ``samples`` area-weighted points of ``a``
    (``sample_meshes``, face normals, stream indices ``[0, samples)``) measured against ``b`` with ``RayGrid.closest`` on
    ``bounding_grid([b], cells)``, and as many of ``b`` (indices ``[samples, 2 samples)``: the two draws are disjoint) against ``a``.
    Unlike ``Mesh.distance_to``, which looks from the VERTICES of one mesh - few and at the cluster representatives after a
    simplification, exactly the points that moved after a smoothing, dense where the triangles are small -, every part of either
    surface counts by its area here; ``distance_to`` stays the cheap one-sided check.

    ``max_distance`` bounds the search as in ``closest`` and has no default; a sample with nothing within it is a MISS, left out of
    the means and counted.  ``thresholds``: distances for which the share of samples within them - precision, recall, F-score - is
    reported; one above ``max_distance`` raises, because misses could not be told from samples beyond it.  The reductions are torch
    expressions in fp64 on the device; two grid builds (one read-back each, plus ``bounding_grid``'s) are the host synchronisations,
    and ``MeshDeviation.report()`` is the read-back of the result.  There is no CPU fallback."""
    if not isinstance(a, Mesh) or not isinstance(b, Mesh):
        raise ValueError("compare_meshes compares two Mesh objects")
    try:
        samples = operator.index(samples)
    except TypeError:
        raise ValueError(f"samples must be an integer >= 1, got {samples!r}") from None
    if samples < 1:
        raise ValueError(f"samples must be an integer >= 1, got {samples}")
    max_distance = float(max_distance)
    if math.isnan(max_distance) or max_distance < 0:
        raise ValueError(f"max_distance must be >= 0 and not NaN, got {max_distance}")
    thresholds = tuple(float(t) for t in thresholds)
    for t in thresholds:
        if math.isnan(t) or t < 0 or t > max_distance:
            raise ValueError(f"a threshold must lie in [0, max_distance = {max_distance}] - beyond it a miss cannot be told from a "
                             f"sample that is merely farther -, got {t}")
    if not all(m.vertices.is_cuda and m.triangles.is_cuda for m in (a, b)):
        raise RuntimeError(NO_CPU)
    from_a = sample_meshes([a], samples, seed=seed, first=0, normals="face", features=False)[0]
    from_b = sample_meshes([b], samples, seed=seed, first=samples, normals="face", features=False)[0]
    grid_a = RayGrid.build([a], *bounding_grid([a], cells))
    grid_b = RayGrid.build([b], *bounding_grid([b], cells))
    a_to_b, distance_a = _one_sided_deviation(from_a, b, grid_b, max_distance, thresholds)
    b_to_a, distance_b = _one_sided_deviation(from_b, a, grid_a, max_distance, thresholds)
    return MeshDeviation(a_to_b, b_to_a, distance_a, distance_b, thresholds)


def intersect_struct(vertices: torch.Tensor, triangles: torch.Tensor, vertex_offsets: torch.Tensor, triangle_offsets: torch.Tensor,
                     total_vertices: int, total_triangles: int, origin, cell, cells, cell_offsets: torch.Tensor, *,
                     references: Optional[torch.Tensor] = None, q_vertices: Optional[torch.Tensor] = None,
                     q_triangles: Optional[torch.Tensor] = None, q_vertex_offsets: Optional[torch.Tensor] = None,
                     q_triangle_offsets: Optional[torch.Tensor] = None, q_total_vertices: Optional[int] = None,
                     q_total_triangles: Optional[int] = None, transform: Optional[torch.Tensor] = None,
                     count: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                     pair_offsets: Optional[torch.Tensor] = None, pairs: Optional[torch.Tensor] = None,
                     segments: Optional[torch.Tensor] = None, self_: bool = False) -> _lib.MeshIntersect:
    """``pr_mesh_intersect_t`` over prepared tensors (fp32 / int32, contiguous, one device); ``max_references`` is the rows of
    ``references``, ``max_pairs`` the rows of ``pairs``.  The query totals default to the targets' with ``self_`` and to the rows of the
    query tensors otherwise."""
    s = _lib.MeshIntersect()
    _set_mesh_header(s, vertex_offsets, total_vertices, total_triangles, _lib.INTERSECT_SELF if self_ else 0)
    _set_grid(s, origin, cell, cells)
    s.max_references = 0 if references is None else references.size(0)
    if q_total_vertices is None:
        q_total_vertices = total_vertices if self_ else (0 if q_vertices is None else q_vertices.size(0))
    if q_total_triangles is None:
        q_total_triangles = total_triangles if self_ else (0 if q_triangles is None else q_triangles.size(0))
    s.q_total_vertices = int(q_total_vertices)
    s.q_total_triangles = int(q_total_triangles)
    s.max_pairs = 0 if pairs is None else pairs.size(0)
    return _set_pointers(s, vertices=vertices, triangles=triangles, vertex_offsets=vertex_offsets, triangle_offsets=triangle_offsets,
                         cell_offsets=cell_offsets, references=references, q_vertices=q_vertices, q_triangles=q_triangles,
                         q_vertex_offsets=q_vertex_offsets, q_triangle_offsets=q_triangle_offsets, transform=transform, count=count,
                         first=first, pair_offsets=pair_offsets, pairs=pairs, segments=segments)


@dataclass
class MeshContacts:
    """What ``RayGrid.intersect`` returns per group, on the device (``pr_mesh_intersect``, include/playrender.h): ``count (QT)`` int32 -
    the target triangles every query triangle cuts -, ``first (QT)`` int32 - the lowest of them, or -1 -, ``offsets (QT + 1)`` int32 -
    the exclusive sums of ``count`` -, ``pairs (P, 2)`` int32 = (query, target) sorted by (query, target), or None, and ``segments
    (P, 2, 3)`` - one contact segment per pair, in the targets' frame - or None.  ``symmetric``: the result of a self-intersection
    query, in which every unordered pair shows up twice.  ``report()`` reads the summary back."""
    count: torch.Tensor
    first: torch.Tensor
    offsets: torch.Tensor
    pairs: Optional[torch.Tensor] = None
    segments: Optional[torch.Tensor] = None
    symmetric: bool = False

    def report(self) -> dict:
        """``pairs`` (unordered pairs for a self-intersection query), ``query_triangles`` - query triangles that cut something -,
        ``target_triangles`` - target triangles that are cut (None without ``pairs``) -, ``contact_length`` - the fp64 sum of the
        segment lengths (None without ``segments``; halved for a self-intersection query) - and ``intersecting``.  ONE read-back."""
        count = self.count.to(torch.int64)
        values = [count.sum().to(torch.float64), (count > 0).sum().to(torch.float64)]
        if self.pairs is not None:
            targets = torch.sort(self.pairs[:, 1]).values                    # (distinct values counted on the device: no shape to read back)
            values.append(((targets[1:] != targets[:-1]).sum() + min(targets.numel(), 1)).to(torch.float64))
        if self.segments is not None:
            d = self.segments.to(torch.float64)
            values.append((d[:, 1] - d[:, 0]).square().sum(dim=1).sqrt().sum())
        values = torch.stack(values).cpu().tolist()                          # (the host synchronisation)
        share = 2 if self.symmetric else 1
        pairs = int(values[0]) // share
        out = {"pairs": pairs, "query_triangles": int(values[1]), "target_triangles": None, "contact_length": None,
               "intersecting": pairs > 0}
        at = 2
        if self.pairs is not None:
            out["target_triangles"] = int(values[at])
            at += 1
        if self.segments is not None:
            out["contact_length"] = values[at] / share
        return out


def _pose_rows(transform, groups: int, dev) -> Optional[torch.Tensor]:
    """``transform`` as ``(G, 3, 4)`` fp32 rows: one ``(3, 4)`` / ``(4, 4)`` matrix for every group, or ``(G, 3, 4)`` / ``(G, 4, 4)``."""
    if transform is None:
        return None
    m = torch.as_tensor(transform, dtype=torch.float32, device=dev)
    if m.dim() == 2:
        m = m.unsqueeze(0).expand(groups, -1, -1)
    if m.dim() != 3 or m.size(0) != groups or m.size(1) not in (3, 4) or m.size(2) != 4:
        raise ValueError(f"transform must be (3, 4), (4, 4), (G, 3, 4) or (G, 4, 4) with G = {groups}, got {list(m.shape)}")
    return m[:, :3, :].contiguous()


@dataclass
class Collision:
    """What ``collide`` returns: ``intersecting`` - the surfaces cut each other -, ``pairs`` - in how many triangle pairs -, and
    ``b_in_a`` - b's first finite vertex lies inside a (None unless asked for)."""
    intersecting: bool
    pairs: int
    b_in_a: Optional[bool] = None


def collide(a, b: Mesh, *, transform=None, cells=32, inside: bool = False) -> Collision:
    """Whether the mesh ``b``, posed by ``transform`` (``v' = R v + t``, a ``(3, 4)`` or ``(4, 4)`` matrix into a's frame, or None),
    cuts ``a`` - a ``Mesh``, sorted into ``bounding_grid([a], cells)`` here, or a ``RayGrid`` of one group that was built once for a
    static object.  ``intersecting`` comes from ``RayGrid.intersect`` and sees every contact of the two SURFACES, including those in
    which no vertex of either mesh lies inside the other; a mesh swallowed whole touches nothing, so ``inside=True`` also reports
    ``b_in_a``: ``contains`` of b's first finite posed vertex on a's grid.  That needs what ``contains`` needs of ``a`` - a capped mesh
    (``close_border=True``) that kept its duplicates when simplified; ``a.audit().report()["balanced"]`` checks it.  A composition:
    one counting call, one ``pr_inside_query`` with ``inside`` (``contains`` does not synchronise), and ONE read-back of both answers;
    a ``Mesh`` given as ``a`` costs the read-backs of ``bounding_grid`` and ``RayGrid.build`` in front of that."""
    if not isinstance(b, Mesh):
        raise ValueError("collide needs a Mesh as its second argument")
    if isinstance(a, Mesh):
        if not (a.vertices.is_cuda and b.vertices.is_cuda):
            raise RuntimeError(NO_CPU)
        a = RayGrid.build([a], *bounding_grid([a], cells))
    if a.groups != 1:
        raise ValueError(f"collide needs a grid of one group, got {a.groups}")
    contacts = a.intersect([b], transform=transform)[0]
    values = [contacts.count.to(torch.int64).sum()]
    if inside:
        m = _pose_rows(transform, 1, a.vertices.device)
        v = b.vertices.detach().to(device=a.vertices.device, dtype=torch.float32).reshape(-1, 3)
        if m is not None:
            v = v @ m[0, :, :3].T + m[0, :, 3]
        if v.size(0) == 0:
            values.append(torch.zeros((), dtype=torch.int64, device=a.vertices.device))
        else:
            finite = torch.isfinite(v).all(dim=1)
            at = torch.argmax(finite.to(torch.uint8))                      # (the first finite vertex)
            point = torch.where(finite[at], v[at], torch.full_like(v[at], math.inf))
            values.append(a.contains(point.reshape(1, 1, 3))[0, 0].to(torch.int64))
    values = torch.stack(values).cpu().tolist()                            # (the host synchronisation)
    return Collision(values[0] > 0, int(values[0]), bool(values[1]) if inside else None)


def bounding_grid(meshes: Sequence[Mesh], cells):
    """A grid of ``cells`` cells (one integer, or three) around the joint bounding box of the meshes' finite vertices, for
    ``RayGrid.build``: per axis ``cell = extent / (cells - 1/4)`` and ``origin = lowest - cell / 8`` - the box is widened by an eighth
    of a cell on every side, so that no vertex lies on its faces and no triangle's padded box (a sixteenth of a cell) leaves it.  An
    axis without extent gets the extent ``2^-10 max(1, |lowest|)``.  Reads the box back: one host synchronisation."""
    meshes = list(meshes)
    try:
        cells = [operator.index(cells)] * 3
    except TypeError:
        cells = [operator.index(n) for n in cells]
    if not all(m.vertices.is_cuda for m in meshes):
        raise RuntimeError(NO_CPU)
    rows = [m.vertices.detach().to(torch.float32).reshape(-1, 3) for m in meshes if m.vertices.numel()]
    if not rows:
        raise ValueError("bounding_grid needs at least one vertex")
    v = torch.cat(rows)
    finite = torch.isfinite(v)
    box = torch.stack([torch.where(finite, v, torch.full_like(v, math.inf)).amin(0),
                       torch.where(finite, v, torch.full_like(v, -math.inf)).amax(0)]).cpu().tolist()      # (the host synchronisation)
    origin, cell = [], []
    for a in range(3):
        lowest, highest = box[0][a], box[1][a]
        if not lowest <= highest:
            raise ValueError("bounding_grid needs a finite vertex on every axis")
        extent = max(highest - lowest, 2.0 ** -10 * max(1.0, abs(lowest)))
        cell.append(extent / (cells[a] - 0.25))
        origin.append(lowest - cell[a] / 8)
    return _ray_grid(origin, cell, cells)


def extract_surface(sigma: torch.Tensor, axes: Sequence[torch.Tensor], level: float, *, normals: bool = True, keep_largest: int = 0,
                    min_points: int = 0, close_border: bool = False, simplify: int = 0, keep_duplicates: bool = False,
                    weld: bool = False, smooth: int = 0, placement: str = "mean") -> List[Mesh]:
    """Meshes of the level set ``sigma = level`` of ``sigma (G, nx, ny, nz)`` (device tensor, z fastest - what ``density_grid``
    returns); ``axes``: the coordinates of the lattice points along x, y, z (``nx``, ``ny``, ``nz`` values).  Returns G meshes.

    Two calls on the current stream: a count-only one, then - after reading the two totals back, the ONE host synchronisation of
    this function - an emitting one into exactly sized tensors.

    ``keep_largest`` / ``min_points`` / ``close_border``: with any of them set the lattice goes through ``clean_lattice`` (fill =
    ``level``) first - floaters are dropped, the surface is capped at the lattice border.  Positions and triangles of the kept
    components do not change; normals near a removed component can, because the gradient stencil reads the blanked values.

    ``simplify = k >= 1``: the meshes are then clustered (``simplify_meshes``) on the grid aligned with the lattice whose cells span
    ``k`` lattice steps (``lattice_cluster_grid``) - evaluate the field finely, keep a mesh of a coarser lattice's size.  Two more
    read-backs (the ends of the axes, the simplified sizes).  At 0 (the default) nothing changes.  ``keep_duplicates`` is
    ``simplify_meshes``'s: duplicate triangles stay, so that every directed edge keeps its partner - what ``RayGrid.winding`` /
    ``contains`` need of a simplified mesh.  ``placement`` is ``simplify_meshes``'s too: ``"quadric"`` moves the clusters' vertices from
    the mean onto the edges and corners that their triangles' planes meet in (no further read-back); it means nothing without
    ``simplify``.

    ``weld=True``: the meshes - after the simplification, if any - go through ``weld_meshes``: one vertex per value, no unreferenced
    vertex, no dropped triangle.  One more read-back.  At False (the default) nothing changes.

    ``smooth = n >= 1``: implies ``weld=True``; the welded meshes then go through ``smooth_meshes(iterations=n, weld=False)`` - ``n``
    Taubin iterations at the default factors, borders pinned, normals recomputed from the smoothed triangles when ``normals`` is set.
    No further read-back.  At 0 (the default) nothing changes."""
    if not sigma.is_cuda:
        raise RuntimeError(NO_CPU)
    if sigma.dim() != 4:
        raise ValueError(f"sigma must be (G, nx, ny, nz), got {list(sigma.shape)}")
    if len(axes) != 3:
        raise ValueError("axes must be the three coordinate vectors of the lattice")
    try:
        simplify = operator.index(simplify)
    except TypeError:
        raise ValueError(f"simplify must be an integer >= 0, got {simplify!r}") from None
    if simplify < 0:
        raise ValueError(f"simplify must be an integer >= 0, got {simplify}")
    try:
        smooth = operator.index(smooth)
    except TypeError:
        raise ValueError(f"smooth must be an integer >= 0, got {smooth!r}") from None
    if smooth < 0 or 2 * smooth > _lib.SMOOTH_MAX_STEPS:
        raise ValueError(f"smooth must be an integer in 0 .. {_lib.SMOOTH_MAX_STEPS // 2}, got {smooth}")
    _placement(placement)
    if smooth:
        meshes = extract_surface(sigma, axes, level, normals=normals, keep_largest=keep_largest, min_points=min_points,
                                 close_border=close_border, simplify=simplify, keep_duplicates=keep_duplicates, weld=True,
                                 placement=placement)
        return smooth_meshes(meshes, iterations=smooth, weld=False, normals=bool(normals))
    dev = sigma.device
    sigma = sigma.detach().to(torch.float32).contiguous()
    if keep_largest or min_points or close_border:
        sigma, _ = clean_lattice(sigma, level, keep_largest=keep_largest, min_points=min_points, close_border=close_border)
    axes = [torch.as_tensor(a).detach().to(device=dev, dtype=torch.float32).contiguous() for a in axes]
    for a in range(3):
        if axes[a].dim() != 1 or axes[a].numel() != sigma.size(1 + a):
            raise ValueError(f"axes[{a}] must hold {sigma.size(1 + a)} coordinates, got {list(axes[a].shape)}")
    G = sigma.size(0)
    with torch.cuda.device(dev):
        offsets = torch.empty((2, G + 1), dtype=torch.int32, device=dev)
        workspace, size = _call_with_workspace("pr_surface_workspace_size", "pr_extract_surface",
                                               surface_struct(sigma, axes, level, offsets[0], offsets[1]), dev)
        vertex_offsets, triangle_offsets = offsets.cpu().tolist()           # (the host synchronisation)
        V, T = vertex_offsets[G], triangle_offsets[G]
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        vertex_normals = torch.empty((V, 3), dtype=torch.float32, device=dev) if normals else None
        triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
        if V > 0:
            emit = surface_struct(sigma, axes, level, offsets[0], offsets[1], vertices, vertex_normals, triangles)
            _call("pr_extract_surface", emit, workspace, size, dev)
    if simplify:                                                   # (the mesher's output is packed already: no Mesh objects in between)
        grid = _cluster_grid(*lattice_cluster_grid(axes, simplify))
        meshes = _simplify_packed(_packed(vertices, triangles, vertex_offsets, triangle_offsets, vertex_normals), *grid, bool(keep_duplicates),
                                  placement)
        return weld_meshes(meshes) if weld else meshes
    if weld:
        return _weld_packed(_packed(vertices, triangles, vertex_offsets, triangle_offsets, vertex_normals), True, False)[0]
    meshes = []
    for g in range(G):
        v0, v1, t0, t1 = vertex_offsets[g], vertex_offsets[g + 1], triangle_offsets[g], triangle_offsets[g + 1]
        meshes.append(Mesh(vertices[v0:v1], triangles[t0:t1], vertex_normals[v0:v1] if normals else None))
    return meshes

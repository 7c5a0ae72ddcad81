"""Mesh intersection without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_mesh_intersect (symbols, struct size, every
refusal), the Python argument errors, and the properties of the exhaustive numpy rule the GPU tests compare against
(tests/intersect_reference.py) on the meshes of tests/surface_reference.py - the pair counts DESIGN.md 28 records, symmetry, self mode,
the regression the conditioning clause exists for, the planes and the length of the contact segments."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, surface
from tests import intersect_reference as ir
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
POINTERS = ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "cell_offsets", "references", "q_vertices", "q_triangles",
            "q_vertex_offsets", "q_triangle_offsets", "transform", "count", "first", "pair_offsets", "pairs", "segments")
QUERY_POINTERS = ("q_vertices", "q_triangles", "q_vertex_offsets", "q_triangle_offsets")


def valid_struct(groups=2, V=1000, T=2000, QV=500, QT=700, cells=(5, 6, 7), max_references=5000, max_pairs=300):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.MeshIntersect()
    s.groups, s.total_vertices, s.total_triangles, s.max_references = groups, V, T, max_references
    s.q_total_vertices, s.q_total_triangles, s.max_pairs = QV, QT, max_pairs
    for a in range(3):
        s.origin[a], s.cell[a], s.cells[a] = -1.0, 0.25, cells[a]
    for k, name in enumerate(POINTERS):
        setattr(s, name, 256 * (k + 1))
    return s


def self_struct(**kw):
    s = valid_struct(**kw)
    s.flags = _lib.INTERSECT_SELF
    s.q_total_vertices, s.q_total_triangles, s.transform = s.total_vertices, s.total_triangles, None
    for name in QUERY_POINTERS:
        setattr(s, name, None)
    return s


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    for name in ("pr_mesh_intersect", "pr_mesh_intersect_workspace_size"):
        assert getattr(built_library, name) is not None and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_mesh_intersect_t" in header and "sizeof(pr_mesh_intersect_t) = 200" in header
    assert "#define PR_INTERSECT_SELF 1u" in header and _lib.INTERSECT_SELF == 1
    # four int32 | origin, cell, cells | capacity, two query totals, max_pairs, reserved | sixteen pointers
    assert C.sizeof(_lib.MeshIntersect) == 16 + 36 + 20 + 16 * 8 == 200
    assert _lib.MeshIntersect.vertices.offset == 72 and _lib.MeshIntersect.segments.offset == 192
    assert C.sizeof(_lib.Closest) == 152 and built_library.pr_abi_version() == 5       # additive: the other structs and the ABI are as they were


def _break(field, value):
    def edit(s):
        setattr(s, field, value)
    return edit


def _break_index(field, index, value):
    def edit(s):
        getattr(s, field)[index] = value
    return edit


def _both(*edits):
    def edit(s):
        for e in edits:
            e(s)
    return edit


REFUSALS = [
    ("null_vertices", _break("vertices", None), b"NULL vertices"),
    ("null_triangles", _break("triangles", None), b"NULL triangles"),
    ("null_vertex_offsets", _break("vertex_offsets", None), b"NULL offsets"),
    ("null_triangle_offsets", _break("triangle_offsets", None), b"NULL offsets"),
    ("null_cell_offsets", _break("cell_offsets", None), b"NULL cell_offsets"),
    ("null_references", _break("references", None), b"NULL references"),
    ("no_groups", _break("groups", 0), b"groups 0"),
    ("no_cells", _break_index("cells", 1, 0), b"cells[1] = 0"),
    ("too_many_cells_on_an_axis", _break_index("cells", 0, 1025), b"cells[0] = 1025"),
    ("too_many_cells", _both(_break_index("cells", 0, 128), _break_index("cells", 1, 128), _break_index("cells", 2, 129)), b"at most 2^21"),
    ("zero_cell", _break_index("cell", 0, 0.0), b"cell[0] = 0"),
    ("nan_cell", _break_index("cell", 2, float("nan")), b"cell[2]"),
    ("inf_cell", _break_index("cell", 2, float("inf")), b"cell[2]"),
    ("nan_origin", _break_index("origin", 0, float("nan")), b"origin[0]"),
    ("inf_origin", _break_index("origin", 2, float("-inf")), b"origin[2]"),
    ("unknown_flag", _break("flags", 2), b"flags 0x2"),
    ("negative_capacity", _break("max_references", -1), b"negative capacity"),
    ("negative_max_pairs", _break("max_pairs", -1), b"negative capacity"),
    ("negative_vertex_total", _break("total_vertices", -1), b"negative total"),
    ("negative_triangle_total", _break("total_triangles", -1), b"negative total"),
    ("negative_query_vertex_total", _break("q_total_vertices", -1), b"negative total"),
    ("negative_query_triangle_total", _break("q_total_triangles", -1), b"negative total"),
    ("null_q_vertices", _break("q_vertices", None), b"NULL q_vertices"),
    ("null_q_triangles", _break("q_triangles", None), b"NULL q_triangles"),
    ("null_q_vertex_offsets", _break("q_vertex_offsets", None), b"NULL offsets (q_"),
    ("null_q_triangle_offsets", _break("q_triangle_offsets", None), b"NULL offsets (q_"),
    ("null_count", _break("count", None), b"NULL count"),
    ("segments_without_pairs", _break("pairs", None), b"segments needs pairs"),
    ("triangle_total_too_large", _break("total_triangles", 2 ** 31 - 512), b"below 2^31"),
    ("query_total_too_large", _break("q_total_triangles", 2 ** 31 - 512), b"below 2^31"),
    ("groups_times_cells_too_large", _both(_break("groups", 2 ** 22), _break_index("cells", 0, 1024)), b"below 2^31"),
]
SELF_REFUSALS = [
    ("self_with_transform", _break("transform", 4096), b"with a transform"),
    ("self_with_foreign_vertices", _break("q_vertices", 4096), b"foreign query pointers"),
    ("self_with_foreign_triangles", _break("q_triangles", 4096), b"foreign query pointers"),
    ("self_with_foreign_vertex_offsets", _break("q_vertex_offsets", 4096), b"foreign query pointers"),
    ("self_with_foreign_triangle_offsets", _break("q_triangle_offsets", 4096), b"foreign query pointers"),
    ("self_with_other_totals", _break("q_total_triangles", 5), b"other query totals"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS + SELF_REFUSALS, ids=[r[0] for r in REFUSALS + SELF_REFUSALS])
def test_refusals_precede_device_work(built_library, name, edit, message):
    """Each broken description is refused with PR_ERR_INVALID and its message by both entry points; the pointers are dummies, so a
    call that got past the checks would not survive."""
    s = self_struct() if name.startswith("self_") else valid_struct()
    edit(s)
    size = C.c_size_t()
    for entry in (lambda: built_library.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)),
                  lambda: built_library.pr_mesh_intersect(C.byref(s), 256, 1 << 40, None)):
        assert entry() == PR_ERR_INVALID
        assert message in built_library.pr_last_error(), built_library.pr_last_error()


def test_the_largest_descriptions_and_the_workspace(built_library):
    lib = built_library
    size = C.c_size_t()
    assert lib.pr_mesh_intersect_workspace_size(None, C.byref(size)) == PR_ERR_INVALID
    assert lib.pr_mesh_intersect_workspace_size(C.byref(valid_struct()), None) == PR_ERR_INVALID
    s = valid_struct(groups=3, QT=700)
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == 0, lib.pr_last_error()
    up = lambda n: (n + 255) // 256 * 256
    assert size.value == 5 * up(4 * 4) + up(4 * 701) + 2 * up(4 * (700 // 256 + 1)) + up(4)               # the header's formula
    for workspace, given, message in ((None, size.value, b"NULL workspace"), (128, size.value, b"256-byte aligned"),
                                      (256, size.value - 1, b"workspace too small")):
        assert lib.pr_mesh_intersect(C.byref(s), workspace, given, None) == PR_ERR_INVALID and message in lib.pr_last_error()
    s = valid_struct(groups=1, V=2 ** 31 - 1, T=2 ** 31 - 257, QV=2 ** 31 - 1, QT=2 ** 31 - 257, cells=(128, 128, 128))
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == 0, lib.pr_last_error()
    s.q_total_triangles += 1                                            # QT + 256 G = 2^31 exactly
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == PR_ERR_INVALID and b"below 2^31" in lib.pr_last_error()
    # only count is required; no queries, no targets, no references, and self mode with NULL or equal query pointers are valid
    s = valid_struct(QT=0, QV=0, T=0, V=0, max_references=0, max_pairs=0)
    s.references = s.first = s.pair_offsets = s.pairs = s.segments = s.transform = None
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == 0, lib.pr_last_error()
    s = self_struct()
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == 0, lib.pr_last_error()
    for name in QUERY_POINTERS:
        setattr(s, name, getattr(s, name[2:]))
    assert lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)) == 0, lib.pr_last_error()


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    grid = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(2, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    mesh = Mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32))
    for call in (lambda: grid.intersect([mesh]), lambda: grid.intersect(self_=True), lambda: mesh.intersections(mesh),
                 lambda: mesh.intersections(grid), lambda: mesh.self_intersections(), lambda: surface.collide(mesh, mesh),
                 lambda: surface.collide(grid, mesh, inside=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    two = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(3, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    with pytest.raises(ValueError, match="one group"):
        mesh.intersections(two)
    with pytest.raises(ValueError, match="one group"):
        surface.collide(two, mesh)
    with pytest.raises(ValueError, match="Mesh"):
        surface.collide(mesh, grid)
    with pytest.raises(ValueError, match="transform must be"):
        surface._pose_rows(torch.zeros(2, 3, 4), 3, "cpu")
    assert list(surface._pose_rows(torch.eye(4), 3, "cpu").shape) == [3, 3, 4] and surface._pose_rows(None, 3, "cpu") is None
    z, zi = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    offsets = torch.zeros(3, dtype=torch.int32)
    s = surface.intersect_struct(z, zi, offsets, offsets, 3, 1, [0, 1, 2], [1, 2, 3], [4, 5, 6], torch.zeros(242, dtype=torch.int32),
                                 q_vertices=torch.zeros(5, 3), q_triangles=torch.zeros((7, 3), dtype=torch.int32), q_vertex_offsets=offsets,
                                 q_triangle_offsets=offsets, count=torch.zeros(7, dtype=torch.int32), pairs=torch.zeros((9, 2), dtype=torch.int32))
    assert (s.groups, s.q_total_vertices, s.q_total_triangles, s.max_pairs, s.max_references, s.flags, list(s.cells), s.transform, s.segments) == \
        (2, 5, 7, 9, 0, 0, [4, 5, 6], None, None)
    s = surface.intersect_struct(z, zi, offsets, offsets, 3, 1, [0, 1, 2], [1, 2, 3], [4, 5, 6], torch.zeros(242, dtype=torch.int32),
                                 count=torch.zeros(1, dtype=torch.int32), self_=True)
    assert (s.flags, s.q_total_vertices, s.q_total_triangles, s.q_vertices, s.max_pairs) == (1, 3, 1, None, 0)
    report = surface.MeshContacts(torch.tensor([2, 0, 2], dtype=torch.int32), torch.tensor([1, -1, 0], dtype=torch.int32),
                                  torch.tensor([0, 2, 2, 4], dtype=torch.int32), torch.tensor([[0, 1], [0, 4], [2, 0], [2, 1]], dtype=torch.int32),
                                  torch.tensor([[[0, 0, 0], [3, 4, 0]]] * 4, dtype=torch.float32), symmetric=True).report()
    assert report == {"pairs": 2, "query_triangles": 2, "target_triangles": 3, "contact_length": 10.0, "intersecting": True}


# ------------------------------------------------------------------------------------------------ the reference's own properties
SHIFT = (0.3, 0.1, 0.05)
ALIGNED = (0.5, 0.5, 0.0)
CASES = {"sphere9": ("sphere", 9, SHIFT, 768, 180), "sphere17": ("sphere", 17, SHIFT, 2832, 338),
         "aligned17": ("sphere", 17, ALIGNED, 2832, 679), "torus17": ("torus", 17, (0.0, 0.3, 0.4), 2616, 218)}
_MESH, _RESULT = {}, {}


def mesh_of(kind, n):
    if (kind, n) not in _MESH:
        field, axes = (sr.sphere_field if kind == "sphere" else sr.torus_field)(n)
        _MESH[(kind, n)] = ir.packed(sr.extract_surface(field[None], axes, 0.0, normals=False))
    return _MESH[(kind, n)]


def result(name):
    """(target, query, the reference's result) of a case; computed once."""
    if name not in _RESULT:
        kind, n, shift, _, _ = CASES[name]
        target = mesh_of(kind, n)
        query = ir.shifted(target, shift)
        _RESULT[name] = (target, query, ir.intersect(target, query))
    return _RESULT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_reference_pair_counts_symmetry_and_boxes(name):
    """The figures DESIGN.md 28.6 records; swapping the roles transposes the pair set; no pair that the edge tests accept fails BOX -
    the regression the conditioning clause exists for."""
    target, query, got = result(name)
    _, _, _, triangles, pairs = CASES[name]
    assert len(target["triangles"]) == triangles and len(got["pairs"]) == pairs and got["outside_box"] == 0
    assert int(got["count"].sum()) == pairs == int(got["pair_offsets"][-1]) and got["accepted"].min() >= 1 and got["accepted"].max() <= 6
    has = got["count"] > 0
    assert np.array_equal(got["first"][has], got["pairs"][np.concatenate([[True], got["pairs"][1:, 0] != got["pairs"][:-1, 0]]), 1])
    assert bool((got["first"][~has] == -1).all())
    swapped = ir.intersect(query, target)
    order = np.lexsort((got["pairs"][:, 0], got["pairs"][:, 1]))
    assert np.array_equal(got["pairs"][order][:, ::-1], swapped["pairs"])
    print(f"{name}: T {triangles}, pairs {pairs}, accepted tests per pair {np.bincount(got['accepted'], minlength=7).tolist()}")


def test_reference_without_the_clause_accepts_noise():
    """What the clause removes (the issue's figures): pairs of the clean 9^3 sphere with itself that share no vertex, and on the
    lattice-aligned shift pairs whose boxes do not overlap."""
    sphere = mesh_of("sphere", 9)
    assert len(ir.intersect(sphere, self_=True, condition=False)["pairs"]) == 28
    target, query, _ = result("aligned17")
    assert ir.intersect(target, query, condition=False)["outside_box"] == 61


def test_reference_far_apart_and_empty():
    sphere = mesh_of("sphere", 9)
    far = ir.intersect(sphere, ir.shifted(sphere, (2.0, 2.0, 2.0)))
    assert len(far["pairs"]) == 0 and not far["count"].any() and bool((far["first"] == -1).all()) and far["pair_offsets"].tolist() == [0] * 769
    empty = ir.packed({"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32)})
    assert len(ir.intersect(sphere, empty)["pairs"]) == 0 and len(ir.intersect(empty, sphere)["count"]) == 768


@pytest.mark.parametrize("kind,n", [("sphere", 9), ("sphere", 17), ("torus", 17)])
def test_reference_self_mode_on_clean_meshes_is_empty(kind, n):
    got = ir.intersect(mesh_of(kind, n), self_=True)
    assert len(got["pairs"]) == 0 and got["outside_box"] == 0


def test_reference_self_mode_on_two_spheres_in_one_group_is_twice_the_cross_count():
    target, query, cross = result("sphere9")
    two = ir.joined(target, query)
    got = ir.intersect(two, self_=True)
    T = len(target["triangles"])
    assert len(got["pairs"]) == 2 * len(cross["pairs"]) == 360
    first_half = got["pairs"][got["pairs"][:, 0] < T]                     # queries of the first sphere against targets of the second
    assert np.array_equal(first_half - np.array([0, T], dtype=np.int32), ir.intersect(query, target)["pairs"])
    order = np.lexsort((got["pairs"][:, 0], got["pairs"][:, 1]))
    assert np.array_equal(got["pairs"][order][:, ::-1], got["pairs"])     # every unordered pair from both sides


PLANE_MULTIPLE = 1.82       # twice the largest multiple measured on the reference (0.91, the shifted 9^3 sphere)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_segment_endpoints_lie_in_both_planes(name):
    """Float64: every endpoint lies within PLANE_MULTIPLE fp32 epsilons of the extent (the largest coordinate magnitude of the two
    meshes) of the planes of both triangles of its pair; an endpoint pair of one accepted test is one point."""
    target, query, got = result(name)
    extent = max(float(np.abs(target["vertices"]).max()), float(np.abs(query["vertices"]).max()))
    distance = ir.plane_distance(target, query, got)
    multiple = float(distance.max()) / (float(np.finfo(F).eps) * extent)
    print(f"{name}: extent {extent:.4g}, largest plane distance {distance.max():.3g} = {multiple:.3g} eps x extent")
    assert multiple <= PLANE_MULTIPLE
    one = got["accepted"] == 1
    assert np.array_equal(got["segments"][one, 0], got["segments"][one, 1]) and bool(np.any(got["segments"][~one, 0] != got["segments"][~one, 1]))


CONTACT_MARGIN = 0.034      # twice the reference's deviation from the circle at 17^3 (1.68 %); 33^3 deviates by 0.12 %


def test_reference_contact_length_of_two_spheres_against_the_circle():
    """Two spheres of radius r at distance d cut in the circle of radius rho = sqrt(r^2 - d^2 / 4), length 3.82849.  The reference's own
    error sets the margin: its contact length is 3.76424 at 17^3 (-1.68 %) and 3.83292 at 33^3 (+0.12 %) - the mesher's sphere is only
    good to a fraction of a lattice step, and the deviation falls with the step.  Asserted at 17^3: twice the measured
    deviation, 3.4 %.  (Half a lattice step of radius would allow 10.6 %, 0.5 h r / rho^2: far more than the reference needs, and it
    would not notice a few percent of segments lost or shortened.)"""
    r, d = 0.63, math.sqrt(sum(x * x for x in SHIFT))
    rho = math.sqrt(r * r - d * d / 4)
    circle = 2 * math.pi * rho
    _, _, got = result("sphere17")
    length = ir.contact_length(got)
    print(f"contact length {length:.6g}, circle {circle:.6g}, relative {length / circle - 1:+.4f}, margin {CONTACT_MARGIN:.4f}")
    assert abs(length / circle - 1) <= CONTACT_MARGIN


def test_kernels_use_no_scratch(tmp_path):
    """The unit compiled with the Makefile's flags and the compiler's resource-usage remarks: every kernel of it reports 0 bytes of
    private memory per lane (a small array whose element is chosen at run time - the contact segment once was - ends up there, in the
    innermost loop)."""
    import re
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "playableenvironments_amd", "csrc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                          "-I", csrc, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "intersect.hip"), "-o",
                          str(tmp_path / "intersect.o")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = dict(re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", run.stderr, flags=re.S))
    kernels = {name: int(size) for name, size in usage.items() if "k_intersect_" in name}
    assert len(kernels) == 4 and any("k_intersect_walk" in name for name in kernels), usage
    assert all(size == 0 for size in kernels.values()), kernels

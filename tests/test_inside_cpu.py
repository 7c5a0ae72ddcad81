"""Inside / outside queries without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_inside_query (symbol, struct size, a C99
client, every refusal), the Python argument errors, and the properties of the exhaustive numpy sum the GPU tests compare against
(tests/inside_reference.py): zero coverage on every mesh whose directed edges balance, windings of 0 or 1 and agreement of the three
axes away from its surface, the sphere's analytic answer, the lattice's own inside mask at lattice points of the capped noise mesh,
the documented limit on open and duplicate-free simplified meshes - and the kernel's column walk, restated over the build's lists,
against the sum on every (mesh, groups, grid, axis) combination of tests/test_inside_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, surface
from tests import inside_reference as ir
from tests import raycast_reference as rr
from tests import simplify_reference as sp
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
POINTERS = ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "cell_offsets", "references", "points", "winding", "crossings")


def valid_struct(groups=2, V=1000, T=2000, cells=(5, 6, 7), count=100, max_references=5000, axis=2):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.Inside()
    s.groups, s.total_vertices, s.total_triangles, s.count, s.max_references, s.axis = groups, V, T, count, max_references, axis
    for a in range(3):
        s.origin[a], s.cell[a], s.cells[a] = -1.0, 0.25, cells[a]
    for name in POINTERS:
        setattr(s, name, 256)
    return s


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbol_and_struct_size(built_library):
    assert getattr(built_library, "pr_inside_query") is not None and "pr_inside_query" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_inside_t" in header and "sizeof(pr_inside_t) = 136" in header
    # four int32 | origin, cell, cells | capacity, count, axis | nine pointers
    assert C.sizeof(_lib.Inside) == 16 + 36 + 12 + 9 * 8 == 136
    assert C.sizeof(_lib.Closest) == 152 and built_library.pr_abi_version() == 5          # the neighbours and the ABI are as they were


def test_plain_c_client_sees_the_same_struct(built_library, tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    source = tmp_path / "client.c"
    source.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "playrender.h"
int main(void) {
    pr_inside_t s;
    memset(&s, 0, sizeof s);
    if (pr_inside_query(&s, NULL) == 0) return 1;                       /* a zeroed description is refused */
    printf("sizeof(pr_inside_t) %zu, axis at %zu, vertices at %zu, points at %zu, crossings at %zu, refusal: %s\n",
           sizeof(pr_inside_t), offsetof(pr_inside_t, axis), offsetof(pr_inside_t, vertices), offsetof(pr_inside_t, points),
           offsetof(pr_inside_t, crossings), pr_last_error());
    return 0;
}
""")
    lib_dir = os.path.dirname(_lib.library_path())
    binary = tmp_path / "client"
    build = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(source),
                            "-L", lib_dir, "-lplayrender", f"-Wl,-rpath,{lib_dir}", "-o", str(binary)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr[-2000:])
    assert (f"sizeof(pr_inside_t) {C.sizeof(_lib.Inside)}, axis at {_lib.Inside.axis.offset}, vertices at {_lib.Inside.vertices.offset}, "
            f"points at {_lib.Inside.points.offset}, crossings at {_lib.Inside.crossings.offset},") in run.stdout


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
    ("negative_cells", _break_index("cells", 2, -3), b"cells[2] = -3"),
    ("too_many_cells_on_an_axis", _break_index("cells", 0, 1025), b"cells[0] = 1025"),
    ("too_many_cells", _both(_break_index("cells", 0, 128), _break_index("cells", 1, 128), _break_index("cells", 2, 129)), b"at most 2^21"),
    ("zero_cell", _break_index("cell", 0, 0.0), b"cell[0] = 0"),
    ("negative_cell", _break_index("cell", 1, -0.5), b"cell[1] = -0.5"),
    ("nan_cell", _break_index("cell", 2, float("nan")), b"cell[2]"),
    ("inf_cell", _break_index("cell", 2, float("inf")), b"cell[2]"),
    ("nan_origin", _break_index("origin", 0, float("nan")), b"origin[0]"),
    ("inf_origin", _break_index("origin", 2, float("-inf")), b"origin[2]"),
    ("flags", _break("flags", 1), b"flags 0x1"),
    ("axis_three", _break("axis", 3), b"axis 3"),
    ("negative_axis", _break("axis", -1), b"axis -1"),
    ("negative_capacity", _break("max_references", -1), b"negative capacity"),
    ("negative_vertex_total", _break("total_vertices", -1), b"negative total"),
    ("negative_triangle_total", _break("total_triangles", -1), b"negative total"),
    ("negative_count", _break("count", -1), b"negative point count"),
    ("null_points", _break("points", None), b"NULL points"),
    ("null_winding", _break("winding", None), b"NULL winding"),
    ("triangle_total_too_large", _break("total_triangles", 2 ** 31 - 512), b"below 2^31"),
    ("groups_times_cells_too_large", _both(_break("groups", 2 ** 22), _break_index("cells", 0, 1024)), b"below 2^31"),
    ("groups_times_count_too_large", _both(_break("groups", 4), _break("count", 2 ** 29)), b"below 2^31"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_device_work(built_library, name, edit, message):
    """Each broken description is refused with PR_ERR_INVALID and its message; the pointers are dummies, so a call that got past the
    checks would not survive."""
    s = valid_struct()
    edit(s)
    assert built_library.pr_inside_query(C.byref(s), None) == PR_ERR_INVALID
    assert message in built_library.pr_last_error(), built_library.pr_last_error()


def test_the_largest_descriptions_and_empty_calls_are_accepted(built_library):
    lib = built_library
    assert lib.pr_inside_query(None, None) == PR_ERR_INVALID
    # no points: a valid call that launches nothing (the pointers are dummies) - at the largest totals, on every axis, without crossings
    for axis in range(3):
        s = valid_struct(groups=1, V=2 ** 31 - 1, T=2 ** 31 - 257, cells=(128, 128, 128), count=0, axis=axis)
        assert lib.pr_inside_query(C.byref(s), None) == 0, lib.pr_last_error()
    s.total_triangles += 1
    assert lib.pr_inside_query(C.byref(s), None) == PR_ERR_INVALID
    s = valid_struct(cells=(1024, 1024, 2), count=0)
    s.crossings = None
    assert lib.pr_inside_query(C.byref(s), None) == 0, lib.pr_last_error()
    s = valid_struct(count=0, max_references=0)
    s.references = None                                                 # a grid without references has none to give
    assert lib.pr_inside_query(C.byref(s), None) == 0, lib.pr_last_error()
    s = valid_struct(groups=4, count=2 ** 29 - 256)                     # G (N + 256) = 2^31 exactly
    assert lib.pr_inside_query(C.byref(s), None) == PR_ERR_INVALID and b"below 2^31" in lib.pr_last_error()


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    grid = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(2, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    for call in (lambda: grid.winding(torch.zeros(4, 3)), lambda: grid.contains(torch.zeros(4, 3)),
                 lambda: grid.contains(torch.zeros(4, 3), any=True), lambda: grid.signed_distance(torch.zeros(4, 3), max_distance=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        grid.signed_distance(torch.zeros(4, 3))                         # max_distance has no default, as for closest
    with pytest.raises(TypeError):
        grid.winding(torch.zeros(4, 3), 2)                              # axis is a keyword
    s = surface.inside_struct(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                              torch.zeros(3, dtype=torch.int32), 3, 1, [0, 1, 2], [1, 2, 3], [4, 5, 6], torch.zeros(242, dtype=torch.int32),
                              points=torch.zeros(2, 7, 3), axis=1)
    assert (s.groups, s.count, s.max_references, s.flags, s.axis, list(s.cells), s.references, s.crossings) == (2, 7, 0, 0, 1, [4, 5, 6], None, None)
    import inspect
    from playableenvironments_amd import ObjectComposer
    assert inspect.signature(ObjectComposer.extract_mesh).parameters["keep_duplicates"].default is False
    assert inspect.signature(surface.extract_surface).parameters["keep_duplicates"].default is False


# ------------------------------------------------------------------------------------------------ the reference's own properties
def batch(kind, groups=1, n=12, seed=0):
    mesh, axes = ir.mesh_case(kind, groups)
    points, sets = ir.point_batch(mesh, axes, n, [ir.make_grid("k2", axes, mesh), ir.OFF_LATTICE], seed)
    return mesh, axes, points, sets


def test_the_tie_rule_is_antisymmetric_and_the_filter_agrees_with_the_rationals():
    rng = np.random.default_rng(0)
    q = (rng.integers(-4, 5, (4000, 6)) * 0.125).astype(F)              # small dyadic coordinates: every operation below is exact
    t = np.array([0, 0.5, 1, 2], dtype=F)[np.arange(2000) % 4][:, None]
    q[:2000, 4:6] = q[:2000, 0:2] + t * (q[:2000, 2:4] - q[:2000, 0:2])     # p on the line through u and v: E = 0 in these 2 000 rows
    q = np.concatenate([q, rng.uniform(-1, 1, (2000, 6)).astype(F)])
    u, v, p = q[:, 0:2], q[:, 2:4], q[:, 4:6]
    counters = {}
    forward, backward = ir.edge_signs(u, v, p, counters), ir.edge_signs(v, u, p)
    assert np.array_equal(forward, -backward)
    assert np.array_equal(forward == 0, np.all(u == v, axis=1))          # zero only for an edge that projects to a point
    exact = np.array([ir.exact_edge_sign(*u[m], *v[m], *p[m]) for m in range(len(q))])
    assert np.array_equal(forward, exact) and counters["zeros"] >= 2000
    # the perturbation p' = (p_i + eps, p_j + eps^2) with a small real eps on the lattice rows, in rationals
    from fractions import Fraction
    eps = Fraction(1, 2 ** 20)
    for m in range(0, 4000, 7):
        ui, uj, vi, vj, pi, pj = (Fraction(float(x)) for x in q[m])
        e = (vi - ui) * (pj + eps * eps - uj) - (vj - uj) * (pi + eps - ui)
        assert forward[m] == (e > 0) - (e < 0), q[m]


@pytest.mark.parametrize("kind", ir.BALANCED)
def test_reference_balanced_meshes_have_zero_coverage_and_windings_of_zero_or_one(kind):
    mesh, axes, points, sets = batch(kind)
    assert ir.directed_edges_balanced(mesh)
    results = [ir.rule(mesh, points, axis) for axis in range(3)]
    for axis, r in enumerate(results):
        assert not r["coverage"].any(), (kind, axis)
        assert not r["winding"][:, sets["not_finite"]].any() and not r["crossings"][:, sets["not_finite"]].any()
        assert not r["winding"][:, sets["far"]].any() and not r["winding"][:, sets["outside"]].any()
        assert 0 < int(r["winding"][:, sets["uniform"]].sum()) < points.shape[1]
    # the axes agree wherever the point is farther than 2^-10 from the mesh (a condition, not a measurement)
    away = ir.distance_from_mesh(mesh, points) > 2.0 ** -10
    assert away.sum() > points.shape[1] // 2
    # ... and there the winding is 0 or 1.  ON the surface the float64 ahead test decides by rounding which of the triangles around the
    # point count: of the 192 vertex points of the torus in tests/test_inside_gpu.py one gets -1 on axis 0 (three crossings, coverage 0).
    for r in results:
        assert np.isin(r["winding"][away], (0, 1)).all(), kind
    for r in results[1:]:
        assert np.array_equal(r["winding"][away], results[0]["winding"][away]), kind
    differ = int(sum((r["winding"] != results[0]["winding"]).sum() for r in results[1:]))
    print(f"{kind}: {int(away.sum())} of {away.size} points away from the surface; axis disagreements on the surface: {differ}")


def test_reference_rejection_by_boxes_changes_nothing():
    mesh, axes, points, sets = batch("sphere", n=6)
    for axis in range(3):
        fast, full = ir.rule(mesh, points, axis), ir.rule(mesh, points, axis, reject=False)
        for key in ("winding", "crossings", "coverage"):
            assert np.array_equal(fast[key], full[key]), (axis, key)


def test_reference_gives_the_spheres_analytic_answer_away_from_the_surface():
    mesh, axes = ir.mesh_case("sphere", 1)
    rng = np.random.default_rng(5)
    points = rng.uniform(-1, 1, (1, 192, 3)).astype(F)
    radius = np.linalg.norm(points[0].astype(np.float64), axis=1)
    clear = np.abs(radius - 0.63) > 0.02                                # (a chord of the 1/8 lattice sags by less than 0.02)
    assert clear.sum() > 150
    for axis in range(3):
        r = ir.rule(mesh, points, axis)
        assert np.array_equal(r["winding"][0][clear], (radius < 0.63)[clear].astype(np.int32)), axis


@pytest.mark.parametrize("fill", [-1.0, None])
def test_reference_equals_the_lattices_own_mask_at_lattice_points(fill):
    """The capped noise lattice: at a lattice point the winding is ``sigma > level`` of the lattice the mesh came from - with fill =
    level wherever the value is not the level (a point whose value is the level lies on the surface)."""
    raw, capped, level, axes = ir.noise_lattice(0, fill=0.0 if fill is None else fill)
    mesh = sr.extract_surface(capped[None], axes, level)
    mesh = ir.pack([mesh])
    rng = np.random.default_rng(6)
    index = np.stack([rng.integers(0, n, 256) for n in ir.NOISE_SHAPE], axis=1)
    points = np.stack([axes[a][index[:, a]] for a in range(3)], axis=1)[None]
    value = capped[index[:, 0], index[:, 1], index[:, 2]]
    decided = value != F(level)
    assert decided.sum() > 180 and (fill is None or decided.all())
    for axis in range(3):
        r = ir.rule(mesh, points, axis)
        assert np.array_equal(r["winding"][0][decided], (value > F(level))[decided].astype(np.int32)), axis
        assert not r["coverage"].any()


def test_reference_documents_the_limit_on_open_and_duplicate_free_meshes():
    """An open mesh and a simplified mesh without its duplicate triangles leave directed edges unpaired: non-zero coverage."""
    for kind in ("noise", "plane"):
        mesh, axes, points, sets = batch(kind)
        assert not ir.directed_edges_balanced(mesh)
        assert any(ir.rule(mesh, points, axis)["coverage"].any() for axis in range(3)), kind
    raw, capped, level, axes = ir.noise_lattice(0)
    fine = sr.extract_surface(capped[None], axes, level)
    seen = {}
    for keep in (True, False):
        # (four lattice steps per cell: at two, no cluster pair of this lattice receives a triangle twice and the two meshes are one)
        mesh = ir.pack([sp.simplify_mesh(fine, *sp.lattice_grid(axes, 4), keep_duplicates=keep)])
        points, _ = ir.point_batch(mesh, axes, 12, [ir.make_grid("k2", axes, mesh), ir.OFF_LATTICE])
        results = [ir.rule(mesh, points, axis) for axis in range(3)]
        seen[keep] = (ir.directed_edges_balanced(mesh), int(sum(np.count_nonzero(r["coverage"]) for r in results)),
                      sorted(set(np.concatenate([r["winding"].ravel() for r in results]).tolist())))
    print("simplified capped noise (kept, removed): (balanced, points with coverage, windings)", seen)
    assert seen[True][0] and seen[True][1] == 0
    assert not seen[False][0] and seen[False][1] > 0


# ------------------------------------------------------------------------------------------------ the walk restated
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", ir.MESHES)
def test_the_walk_restated_equals_the_sum(kind, groups):
    """The kernel's column walk in numpy against the exhaustive sum, on every grid and axis of the GPU tests (six points per set here;
    the GPU tests use the full sets)."""
    mesh, axes, points, sets = batch(kind, groups, n=6, seed=1)
    wants = [ir.rule(mesh, points, axis) for axis in range(3)]
    walked = 0
    for name in ir.GRIDS:
        grid = ir.make_grid(name, axes, mesh)
        lists = rr.grid_lists(mesh, *grid)
        for axis, want in enumerate(wants):
            got = ir.walk(mesh, *grid, points, axis, lists)
            for key in ("winding", "crossings"):
                assert np.array_equal(got[key], want[key]), (kind, groups, name, axis, key, np.argwhere(got[key] != want[key])[:4])
            walked += int(got["cells_walked"].sum())
            # below the grid along the ray's axis the whole column is walked
            low = [n for n in range(sets["outside"].start, sets["outside"].stop) if (n % 6) // 2 == axis and n % 2 == 0]
            if name == "k2":
                assert np.all(got["cells_walked"][:, low] == grid[2][axis])
    assert walked > 0 and all(want["crossings"].sum() > 0 for want in wants)

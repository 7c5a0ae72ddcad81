"""Closest-point queries without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_closest_query (symbol, struct size, a C99
client, every refusal), the Python argument errors, and the properties of the exhaustive numpy search the GPU tests compare against
(tests/closest_reference.py) on the 17^3 sphere of tests/surface_reference.py - with the conditions the GPU suite relies on: ties in
ordinary sets, every region of the walk taken, a finite radius that splits a set."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, surface
from tests import closest_reference as cr
from tests import raycast_reference as rr
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
POINTERS = ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "cell_offsets", "references", "points", "distance", "triangle",
            "point", "barycentric")


def valid_struct(groups=2, V=1000, T=2000, cells=(5, 6, 7), count=100, max_references=5000):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.Closest()
    s.groups, s.total_vertices, s.total_triangles, s.count, s.max_references = groups, V, T, count, max_references
    s.max_distance = math.inf
    for a in range(3):
        s.origin[a], s.cell[a], s.cells[a] = -1.0, 0.25, cells[a]
    for name in POINTERS:
        setattr(s, name, 256)
    return s


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbol_and_struct_size(built_library):
    assert getattr(built_library, "pr_closest_query") is not None and "pr_closest_query" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_closest_t" in header and "sizeof(pr_closest_t) = 152" in header
    # four int32 | origin, cell, cells | capacity, count, max_distance | eleven pointers
    assert C.sizeof(_lib.Closest) == 16 + 36 + 12 + 11 * 8 == 152
    assert C.sizeof(_lib.Raycast) == 160 and built_library.pr_abi_version() == 5          # the ray cast's struct and the ABI are as they were


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
    pr_closest_t s;
    memset(&s, 0, sizeof s);
    if (pr_closest_query(&s, NULL) == 0) return 1;                      /* a zeroed description is refused */
    printf("sizeof(pr_closest_t) %zu, max_distance at %zu, vertices at %zu, points at %zu, barycentric at %zu, refusal: %s\n",
           sizeof(pr_closest_t), offsetof(pr_closest_t, max_distance), offsetof(pr_closest_t, vertices), offsetof(pr_closest_t, points),
           offsetof(pr_closest_t, barycentric), pr_last_error());
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
    assert (f"sizeof(pr_closest_t) {C.sizeof(_lib.Closest)}, max_distance at {_lib.Closest.max_distance.offset}, vertices at "
            f"{_lib.Closest.vertices.offset}, points at {_lib.Closest.points.offset}, barycentric at {_lib.Closest.barycentric.offset},") in run.stdout


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
    ("negative_capacity", _break("max_references", -1), b"negative capacity"),
    ("negative_vertex_total", _break("total_vertices", -1), b"negative total"),
    ("negative_triangle_total", _break("total_triangles", -1), b"negative total"),
    ("negative_count", _break("count", -1), b"negative point count"),
    ("nan_max_distance", _break("max_distance", float("nan")), b"max_distance"),
    ("negative_max_distance", _break("max_distance", -0.5), b"max_distance -0.5"),
    ("negative_infinite_max_distance", _break("max_distance", float("-inf")), b"max_distance"),
    ("null_points", _break("points", None), b"NULL points"),
    ("null_distance", _break("distance", None), b"NULL distance"),
    ("point_without_triangle", _both(_break("triangle", None), _break("barycentric", None)), b"point needs triangle"),
    ("barycentric_without_triangle", _both(_break("triangle", None), _break("point", None)), b"barycentric needs triangle"),
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
    assert built_library.pr_closest_query(C.byref(s), None) == PR_ERR_INVALID
    assert message in built_library.pr_last_error(), built_library.pr_last_error()


def test_the_largest_descriptions_and_empty_calls_are_accepted(built_library):
    lib = built_library
    assert lib.pr_closest_query(None, None) == PR_ERR_INVALID
    # no points: a valid call that launches nothing (the pointers are dummies) - at the largest totals, radii 0 and +inf, no outputs
    s = valid_struct(groups=1, V=2 ** 31 - 1, T=2 ** 31 - 257, cells=(128, 128, 128), count=0)
    assert lib.pr_closest_query(C.byref(s), None) == 0, lib.pr_last_error()
    s.total_triangles += 1
    assert lib.pr_closest_query(C.byref(s), None) == PR_ERR_INVALID
    s = valid_struct(cells=(1024, 1024, 2), count=0)
    s.max_distance = 0.0
    s.triangle = s.point = s.barycentric = None
    assert lib.pr_closest_query(C.byref(s), None) == 0, lib.pr_last_error()
    s = valid_struct(count=0, max_references=0)
    s.references = None                                                 # a grid without references has none to give
    assert lib.pr_closest_query(C.byref(s), None) == 0, lib.pr_last_error()
    s = valid_struct(groups=4, count=2 ** 29 - 256)                     # G (N + 256) = 2^31 exactly
    assert lib.pr_closest_query(C.byref(s), None) == PR_ERR_INVALID and b"below 2^31" in lib.pr_last_error()


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    grid = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(2, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.closest(torch.zeros(4, 3), max_distance=1.0)
    mesh = Mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.distance_to(mesh, max_distance=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.distance_to(grid, max_distance=1.0)
    with pytest.raises(TypeError):
        grid.closest(torch.zeros(4, 3))                                 # max_distance has no default
    with pytest.raises(TypeError):
        mesh.distance_to(mesh)
    two = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(3, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    with pytest.raises(ValueError, match="one group"):
        mesh.distance_to(two, max_distance=1.0)
    s = surface.closest_struct(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                               torch.zeros(3, dtype=torch.int32), 3, 1, [0, 1, 2], [1, 2, 3], [4, 5, 6], torch.zeros(242, dtype=torch.int32),
                               points=torch.zeros(2, 7, 3), max_distance=2.5)
    assert (s.groups, s.count, s.max_references, s.flags, s.max_distance, list(s.cells), s.references, s.point) == (2, 7, 0, 0, 2.5, [4, 5, 6], None, None)


# ------------------------------------------------------------------------------------------------ the reference's own properties
N = 1024
GRID = ([-1.0] * 3, [0.25] * 3, [8, 8, 8])                              # the lattice grid at two steps
OFF_LATTICE = ([-0.7, -0.71, -0.69], [0.11, 0.13, 0.17], [13, 11, 9])


@pytest.fixture(scope="module")
def sphere():
    field, axes = sr.sphere_field(17)
    mesh = sr.extract_surface(field[None], axes, 0.0)
    assert (len(mesh["vertices"]), len(mesh["triangles"])) == (1418, 2832)
    rng = np.random.default_rng(0)
    v = mesh["vertices"]
    sets = {"vertices": v[rng.integers(0, 1418, N)], "radius_3": rr.sphere_origins(rng, N, 3.0), "centre": np.zeros((1, 3), dtype=F),
            "ball": rr.ball_points(rng, N, 1.0)}
    out = {"mesh": mesh, "axes": axes, "points": {k: p[None] for k, p in sets.items()}}
    out["tables"] = {k: cr.pair_table(mesh, p) for k, p in out["points"].items()}
    out["inf"] = {k: cr.closest(mesh, p, np.inf, out["tables"][k]) for k, p in out["points"].items()}
    radii = np.linalg.norm(v.astype(np.float64), axis=1)
    out["radii"] = (radii.min(), radii.max())
    return out


def test_reference_points_on_vertices_tie_and_go_to_the_lowest_index(sphere):
    """A point on a mesh vertex has dist2 == 0 from every triangle around the vertex (q is a copy): at least three tie, and the
    lowest index wins."""
    result = sphere["inf"]["vertices"]
    assert np.all(result["dist2"] == 0) and np.all(result["distance"] == 0) and np.all(result["ties"] >= 3)
    assert np.all(np.isin(result["region"], (0, 1, 3)))                # won as a vertex of the winner
    table, triangles = sphere["tables"]["vertices"][0], sphere["mesh"]["triangles"]
    for i in range(0, N, 16):
        equal = np.nonzero(table["alive"] & (table["dist2"][i] == 0))[0]
        assert len(equal) == result["ties"][0, i] and equal.min() == result["triangle"][0, i]
        assert np.array_equal(result["point"][0, i], sphere["points"]["vertices"][0, i])
    print(f"on vertices: ties {result['ties'].min()} .. {result['ties'].max()}")


def test_reference_distances_from_outside_and_from_the_centre_lie_in_the_meshs_range(sphere):
    low, high = sphere["radii"]
    assert 0.62 <= low and high <= 0.63
    outside = sphere["inf"]["radius_3"]
    assert int((outside["triangle"] < 0).sum()) == 0
    radius = np.linalg.norm(outside["point"][0].astype(np.float64), axis=1)
    # the mesh is inscribed in its vertices' range: a point of a triangle is at most as far from the centre as a vertex, and a chord
    # of a 1/8 lattice sags by less than 0.02
    assert low - 0.02 <= radius.min() and radius.max() <= high + 1e-6
    assert np.all(np.abs(outside["distance"][0] - (3 - radius)) < 0.02)
    centre = sphere["inf"]["centre"]
    assert centre["triangle"][0, 0] >= 0 and low - 0.02 <= centre["distance"][0, 0] <= high
    print(f"closest points seen from radius 3: radii {radius.min():.4f} .. {radius.max():.4f}; from the centre: {centre['distance'][0, 0]:.4f}, "
          f"{centre['ties'][0, 0]} tie")


def test_reference_results_pass_the_float64_check(sphere):
    for name, points in sphere["points"].items():
        for radius in (np.inf, 0.3):
            result = cr.closest(sphere["mesh"], points, radius, sphere["tables"][name])
            worst = cr.check_float64(sphere["mesh"], points, result, radius)
            print(name, radius, worst)
            b = result["barycentric"]
            assert b.min() >= 0 and (b[..., 0] + b[..., 1]).max() <= 1 + 1e-6


def test_reference_finite_radius_splits_a_set_and_zero_keeps_the_surface(sphere):
    points, table = sphere["points"]["ball"], sphere["tables"]["ball"]
    full = sphere["inf"]["ball"]
    within = cr.closest(sphere["mesh"], points, 0.3, table)
    hit = within["triangle"][0] >= 0
    assert 0 < int(hit.sum()) < N                                       # some but not all are misses
    same = lambda key: np.array_equal(within[key][0][hit].view(np.int32), full[key][0][hit].view(np.int32))
    assert same("distance") and same("triangle") and same("point") and same("barycentric")
    assert np.all(full["distance"][0][~hit] > F(0.3)) and np.all(within["distance"][0][~hit] == np.inf)
    assert not within["point"][0][~hit].any() and not within["barycentric"][0][~hit].any()
    zero = cr.closest(sphere["mesh"], sphere["points"]["vertices"], 0.0, sphere["tables"]["vertices"])
    assert np.all(zero["triangle"] >= 0) and int((cr.closest(sphere["mesh"], points, 0.0, table)["triangle"] >= 0).sum()) == 0
    bad = np.array([[[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]], dtype=F)
    none = cr.closest(sphere["mesh"], bad, np.inf)
    assert np.all(none["triangle"] == -1) and np.all(none["distance"] == np.inf)


def test_conditions_of_the_gpu_suite_hold(sphere):
    """What tests/test_closest_gpu.py relies on, checked with the reference alone on its own point sets (the 17^3 sphere, sixteen
    points per set): the vertex set and another ordinary set contain ties; every region of the seven-way walk is taken by some
    (point, triangle) pair and the winners cover vertices, edges and the interior; one cell as the radius turns some but not all
    points of the sets on cell faces and on cell corners into misses."""
    mesh, axes = sphere["mesh"], sphere["axes"]
    points, sets = cr.point_batch(mesh, axes, 16, [GRID, OFF_LATTICE], 2.0 / 64)
    assert points.shape == (1, 192, 3) and list(sets) == list(cr.SETS)
    tables = cr.pair_table(mesh, points)
    full = cr.closest(mesh, points, np.inf, tables)
    ties = {name: int((full["ties"][0, sl] > 1).sum()) for name, sl in sets.items()}
    taken = np.bincount(tables[0]["region"][:, tables[0]["alive"]].ravel(), minlength=7)
    won = np.bincount(full["region"][full["region"] >= 0], minlength=7)
    print("ties per set:", ties, "\nregions of all pairs:", dict(zip(cr.REGIONS, taken.tolist())), "\nregions of the winners:",
          dict(zip(cr.REGIONS, won.tolist())))
    assert ties["vertices"] == 16 and ties["midpoints"] > 0 and ties["centre"] + ties["far"] + ties["corners"] + ties["faces"] > 0
    assert np.all(taken > 0)
    assert won[[0, 1, 3]].sum() > 0 and won[[2, 4, 5]].sum() > 0 and won[6] > 0
    split = cr.closest(mesh, points, 0.25, tables)
    for name in ("faces", "corners"):                                   # points all over the grids' boxes: some within a cell, some not
        assert 0 < int((split["triangle"][0, sets[name]] >= 0).sum()) < 16, name
    assert np.all(split["triangle"][0, sets["quarter"]] >= 0) and np.all(split["triangle"][0, sets["three"]] < 0)
    assert np.all(split["triangle"][0, sets["far"]] < 0)
    assert np.all(full["triangle"][0, sets["not_finite"]] < 0)
    finite = np.ones(192, dtype=bool)
    finite[sets["not_finite"]] = False
    assert np.all(full["triangle"][0, finite] >= 0)
    cr.check_float64(mesh, points, full, np.inf)
    cr.check_float64(mesh, points, split, 0.25)


def test_the_walk_restated_equals_the_search_on_the_sphere(sphere):
    """The kernel's shell walk in numpy against the exhaustive search on two grids and three radii (all combinations of the GPU
    tests were run the same way before the first GPU run: DESIGN.md 22.2); what it visits is counted."""
    mesh, axes = sphere["mesh"], sphere["axes"]
    points, sets = cr.point_batch(mesh, axes, 4, [GRID, OFF_LATTICE], 2.0 / 64)
    inside = np.ones(points.shape[1], dtype=bool)
    inside[sets["beyond"]] = False
    tables = cr.pair_table(mesh, points)
    for grid in (GRID, OFF_LATTICE):
        lists = rr.grid_lists(mesh, *grid)
        for radius in (np.inf, 0.125, 0.25):
            want, got = cr.closest(mesh, points, radius, tables), cr.walk(mesh, *grid, points, radius, tables, lists)
            for key in ("distance", "triangle", "point", "barycentric"):
                assert np.array_equal(got[key][:, inside].view(np.int32), want[key][:, inside].view(np.int32)), (grid[2], radius, key)
            if radius == 0.25 and grid is GRID:                         # one cell as the radius: the walk ends after shell 2 at the latest
                assert got["cells_tested"].max() <= 125

"""The mesh audit without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_mesh_audit (symbols, struct size, a C99 client,
every refusal through both entry points, the largest accepted totals, the workspace formula), the Python argument errors, and the
properties of the numpy restatement the GPU tests compare against (tests/audit_reference.py) on meshes whose answers the project
already records: the sphere's and the torus's counts, Euler characteristics, area and volume, two spheres in one group, the open
plane, the raw and the capped noise mesh, identity by value against identity by index, the off-lattice simplification with and
without its duplicates, agreement with ``inside_reference.directed_edges_balanced`` on all its meshes, and a hand-made hostile
mesh whose counts are derived by hand."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, surface
from tests import audit_reference as ar
from tests import components_reference as cc
from tests import inside_reference as ir
from tests import simplify_reference as sp
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
POINTERS = ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "counts", "measures", "labels")


def valid_struct(groups=2, V=1000, T=2000):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.MeshAudit()
    s.groups, s.total_vertices, s.total_triangles = groups, V, T
    for name in POINTERS:
        setattr(s, name, 256)
    return s


def both_entry_points(lib, s):
    """(status, message) of the host-only entry point and of the call with a NULL workspace, which the call refuses last."""
    size = C.c_size_t(12345)
    first = lib.pr_mesh_audit_workspace_size(C.byref(s), C.byref(size)), lib.pr_last_error()
    second = lib.pr_mesh_audit(C.byref(s), None, 0, None), lib.pr_last_error()
    return first, second, size.value


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    for name in ("pr_mesh_audit", "pr_mesh_audit_workspace_size"):
        assert getattr(built_library, name) is not None and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_mesh_audit_t" in header and "sizeof(pr_mesh_audit_t) = 72" in header
    # four int32 | four input pointers | three output pointers
    assert C.sizeof(_lib.MeshAudit) == 16 + 4 * 8 + 3 * 8 == 72
    assert (_lib.MeshAudit.vertices.offset, _lib.MeshAudit.counts.offset, _lib.MeshAudit.labels.offset) == (16, 48, 64)
    # the neighbours and the ABI are as they were
    assert (C.sizeof(_lib.Inside), C.sizeof(_lib.Closest), C.sizeof(_lib.Raycast), C.sizeof(_lib.Simplify)) == (136, 152, 160, 160)
    assert built_library.pr_abi_version() == 5 and "#define PR_ABI_VERSION 5" in header


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
    pr_mesh_audit_t s;
    size_t bytes = 0;
    memset(&s, 0, sizeof s);
    if (pr_mesh_audit_workspace_size(&s, &bytes) == 0) return 1;        /* a zeroed description is refused */
    if (pr_mesh_audit(&s, NULL, 0, NULL) == 0) return 2;
    printf("sizeof(pr_mesh_audit_t) %zu, flags at %zu, vertices at %zu, triangle_offsets at %zu, counts at %zu, measures at %zu, "
           "labels at %zu, refusal: %s\n", sizeof(pr_mesh_audit_t), offsetof(pr_mesh_audit_t, flags), offsetof(pr_mesh_audit_t, vertices),
           offsetof(pr_mesh_audit_t, triangle_offsets), offsetof(pr_mesh_audit_t, counts), offsetof(pr_mesh_audit_t, measures),
           offsetof(pr_mesh_audit_t, labels), pr_last_error());
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
    M = _lib.MeshAudit
    assert (f"sizeof(pr_mesh_audit_t) {C.sizeof(M)}, flags at {M.flags.offset}, vertices at {M.vertices.offset}, triangle_offsets at "
            f"{M.triangle_offsets.offset}, counts at {M.counts.offset}, measures at {M.measures.offset}, labels at {M.labels.offset},") in run.stdout


def _break(field, value):
    def edit(s):
        setattr(s, field, value)
    return edit


REFUSALS = [
    ("null_vertices", _break("vertices", None), b"NULL vertices"),
    ("null_triangles", _break("triangles", None), b"NULL triangles"),
    ("null_vertex_offsets", _break("vertex_offsets", None), b"NULL offsets"),
    ("null_triangle_offsets", _break("triangle_offsets", None), b"NULL offsets"),
    ("null_counts", _break("counts", None), b"NULL counts"),
    ("no_groups", _break("groups", 0), b"groups 0"),
    ("negative_groups", _break("groups", -2), b"groups -2"),
    ("negative_vertex_total", _break("total_vertices", -1), b"negative total"),
    ("negative_triangle_total", _break("total_triangles", -1), b"negative total"),
    ("flag_bit_0", _break("flags", 1), b"flags 0x1"),
    ("flag_bit_31", _break("flags", 0x80000000), b"flags 0x80000000"),
    ("vertex_total_too_large", _break("total_vertices", 2 ** 30), b"below 2^31"),
    ("triangle_total_too_large", _break("total_triangles", 357913942), b"below 2^31"),
    ("too_many_groups", _break("groups", 2 ** 23), b"below 2^31"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_device_work_in_both_entry_points(built_library, name, edit, message):
    """Each broken description is refused with PR_ERR_INVALID and its message by both entry points; the pointers are dummies, so a
    call that got past the checks would not survive."""
    s = valid_struct()
    edit(s)
    first, second, size = both_entry_points(built_library, s)
    assert first[0] == PR_ERR_INVALID and message in first[1], first
    assert second[0] == PR_ERR_INVALID and message in second[1], second
    assert size == 12345                                                # (nothing was written)


def test_the_call_alone_refuses_the_workspace(built_library):
    lib = built_library
    s = valid_struct()
    size = C.c_size_t()
    assert lib.pr_mesh_audit_workspace_size(C.byref(s), C.byref(size)) == 0
    assert lib.pr_mesh_audit_workspace_size(C.byref(s), None) == PR_ERR_INVALID and b"NULL bytes" in lib.pr_last_error()
    assert lib.pr_mesh_audit_workspace_size(None, C.byref(size)) == PR_ERR_INVALID and lib.pr_mesh_audit(None, None, 0, None) == PR_ERR_INVALID
    assert lib.pr_mesh_audit(C.byref(s), None, size.value, None) == PR_ERR_INVALID and b"NULL workspace" in lib.pr_last_error()
    assert lib.pr_mesh_audit(C.byref(s), 256 + 8, size.value, None) == PR_ERR_INVALID and b"256-byte aligned" in lib.pr_last_error()
    assert lib.pr_mesh_audit(C.byref(s), 256, size.value - 1, None) == PR_ERR_INVALID and b"workspace too small" in lib.pr_last_error()


def test_the_largest_totals_are_accepted_and_the_next_are_not(built_library):
    """2 V + 256 G and 6 T + 256 G stay below 2^31.  The call itself is asked with a NULL workspace, which it refuses last: that
    message says the description passed."""
    lib = built_library
    largest_v, largest_t = (2 ** 31 - 256 - 1) // 2, (2 ** 31 - 256 - 1) // 6
    assert 2 * largest_v + 256 < 2 ** 31 <= 2 * (largest_v + 1) + 256 and 6 * largest_t + 256 < 2 ** 31 <= 6 * (largest_t + 1) + 256
    s = valid_struct(groups=1, V=largest_v, T=largest_t)
    s.measures, s.labels = None, None                                   # both optional
    first, second, size = both_entry_points(lib, s)
    assert first[0] == 0 and second[0] == PR_ERR_INVALID and b"NULL workspace" in second[1], (first, second)
    assert size > 16 * largest_v + 140 * largest_t
    for field, value in (("total_vertices", largest_v + 1), ("total_triangles", largest_t + 1)):
        s = valid_struct(groups=1, V=largest_v, T=largest_t)
        setattr(s, field, value)
        first, second, _ = both_entry_points(lib, s)
        assert first[0] == second[0] == PR_ERR_INVALID and b"below 2^31" in first[1] and b"below 2^31" in second[1], field
    s = valid_struct(groups=3, V=0, T=0)                                # empty input is valid
    assert both_entry_points(lib, s)[0][0] == 0


@pytest.mark.parametrize("G,V,T", [(1, 0, 0), (1, 1, 1), (3, 1000, 2000), (5, 4321, 98765), (2, 256, 512), (64, 63, 65)])
def test_the_workspace_is_the_documented_sum(built_library, G, V, T):
    up = lambda n: (n + 255) // 256 * 256
    BV, BT = (V + 255) // 256 + G, (T + 255) // 256 + G
    want = (4 * up(4 * (G + 1)) + up(8 * V) + 2 * up(4 * V) + 2 * up(48 * T) + up(24 * T) + up(12 * T) + 2 * up(4 * T) + up(40 * BT) +
            up(32 * BT) + up(4 * BV))
    size = C.c_size_t()
    s = valid_struct(G, V, T)
    assert built_library.pr_mesh_audit_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want
    s.measures, s.labels = None, None                                   # (the outputs asked for do not change it)
    assert built_library.pr_mesh_audit_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    mesh = surface.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32))
    grid = surface.RayGrid(torch.zeros(3, 3), None, torch.zeros(2, dtype=torch.int32), None, (0, 0), ([0] * 3, [1] * 3, [1] * 3), None, None)
    for call in (lambda: surface.audit_meshes([mesh]), lambda: surface.audit_meshes([mesh], labels=True), lambda: mesh.audit(),
                 lambda: mesh.audit(labels=True), lambda: mesh.keep_shells(1), lambda: grid.audit()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="at least one mesh"):
        surface.audit_meshes([])
    with pytest.raises(TypeError):
        surface.audit_meshes([mesh], True)                              # labels is a keyword
    for n in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="integer >= 1"):
            mesh.keep_shells(n)
    s = surface.audit_struct(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                             torch.zeros(3, dtype=torch.int32), 3, 1, torch.zeros((2, 12), dtype=torch.int32))
    assert (s.groups, s.total_vertices, s.total_triangles, s.flags, s.measures, s.labels) == (2, 3, 1, 0, None, None)
    assert surface.AUDIT_COUNT_FIELDS == ar.FIELDS and len(ar.FIELDS) == 10 and _lib.AUDIT_COUNTS == 12 and _lib.AUDIT_MEASURES == 8
    for method in (surface.RayGrid.winding, surface.RayGrid.contains, surface.RayGrid.signed_distance):
        assert "RayGrid.audit" in method.__doc__


def test_report_names_the_fields_without_a_gpu():
    """``MeshAudit.report`` on host tensors (it only reads): the reference's numbers in, the reference's dict out."""
    mesh, expected = ar.hand_made()
    want = ar.audit(mesh)
    got = surface.MeshAudit(torch.from_numpy(want["counts"][0]), torch.from_numpy(want["measures"][0])).report()
    assert got == ar.report(want["counts"][0], want["measures"][0])
    assert {k: got[k] for k in expected} == expected and got["balanced"] is False and got["closed_manifold"] is False


# ------------------------------------------------------------------------------------------------ the reference's own properties
def one(mesh):
    """(report dict, reference result) of a single-group mesh."""
    r = ar.audit(mesh)
    return ar.report(r["counts"][0], r["measures"][0]), r


def test_reference_sphere_and_torus_have_the_recorded_counts():
    sphere, _ = ir.part("sphere")
    got, r = one(sphere)
    assert (len(sphere["vertices"]), len(sphere["triangles"])) == (1418, 2832)
    assert (got["vertices"], got["candidates"], got["dropped"], got["edges"]) == (1418, 2832, 0, 4248)
    assert got["balanced"] and got["closed_manifold"] and got["euler_characteristic"] == 2 and got["shells"] == 1 and got["largest_shell"] == 2832
    assert sr.directed_edges_once(sphere["triangles"]) and sr.euler_characteristic(1418, sphere["triangles"]) == 2
    assert not (r["labels"] != 0).any() and not r["counts"][0, 10:].any() and not r["measures"][0, 5:].any()
    torus, _ = ir.part("torus")
    field, axes = sr.torus_field(33)
    torus33 = sr.extract_surface(field[None], axes, 0.0)
    got, _ = one(torus33)
    assert (got["vertices"], got["candidates"]) == (5540, 11080) and got["euler_characteristic"] == 0 and got["closed_manifold"] and got["shells"] == 1
    got, _ = one(torus)
    assert got["euler_characteristic"] == 0 and got["closed_manifold"]


def test_reference_area_and_volume_equal_the_existing_helpers_and_lie_near_the_analytic_values():
    sphere, _ = ir.part("sphere")
    got, r = one(sphere)
    volume, area = sr.signed_volume(sphere["vertices"], sphere["triangles"]), sr.triangle_areas(sphere["vertices"], sphere["triangles"]).sum()
    # two float64 sums of 2 832 terms in different orders, the terms in different association
    assert abs(got["signed_volume"] - volume) <= 2832 * 2.0 ** -52 * r["absolute"][0, 1] and abs(got["area"] - area) <= 2832 * 2.0 ** -52 * area
    radius = 0.63
    assert 0.95 * 4 / 3 * np.pi * radius ** 3 < got["signed_volume"] < 4 / 3 * np.pi * radius ** 3            # (chords: inscribed)
    assert 0.97 * 4 * np.pi * radius ** 2 < got["area"] < 1.01 * 4 * np.pi * radius ** 2
    assert np.abs(got["centroid"]).max() < 1e-6


def test_reference_two_spheres_in_one_group_are_two_shells():
    mesh = ar.two_spheres()
    got, r = one(mesh)
    assert got["shells"] == 2 and got["euler_characteristic"] == 4 and got["closed_manifold"] and got["dropped"] == 0
    assert got["largest_shell"] * 2 == got["candidates"]
    labels, sizes = np.unique(r["labels"], return_counts=True)
    assert labels[0] == 0 and len(labels) == 2 and sizes.tolist() == [got["largest_shell"]] * 2
    # by the x coordinate of a corner: the sphere at -0.47 holds the triangle 0
    side = mesh["vertices"][mesh["triangles"][:, 0], 0] > 0
    assert np.array_equal(r["labels"] == labels[1], side) and r["labels"][np.argmax(side)] == np.argmax(side)
    unequal, _ = one(ar.two_spheres((0.27, 0.36)))
    assert unequal["shells"] == 2 and unequal["largest_shell"] * 2 > unequal["candidates"] and unequal["centroid"][0] > 0.1


def test_reference_open_and_closed_meshes():
    plane, _ = one(ir.part("plane")[0])
    assert plane["boundary_edges"] > 0 and not plane["balanced"] and plane["non_manifold_edges"] == 0 and plane["euler_characteristic"] == 1
    noise, _ = one(ir.part("noise")[0])
    assert not noise["balanced"] and noise["boundary_edges"] > 0
    capped, _ = one(ir.part("capped_noise")[0])
    assert capped["balanced"] and capped["closed_manifold"] and capped["shells"] > 1
    lattice, _ = one(sr.extract_surface(np.array([[[1, 0], [0, 0]], [[0, 0], [0, 1]]], dtype=F)[None], [np.array([0, 1], dtype=F)] * 3, 0.5))
    assert lattice["candidates"] == 12 and lattice["boundary_edges"] == 12 and not lattice["balanced"]


def test_reference_identifies_vertices_by_value():
    """The uncapped lattice with a third of its entries on the level reaches the border and is open by either identity.  Capped, it is
    balanced by value - and by index too (``simplify_reference.directed_edges_balanced``): the mesher's coinciding vertices come with
    the degenerate triangles that pair their edges up.  The case that separates the two identities is therefore hand-made: a
    tetrahedron whose triangles share no vertex index."""
    raw = ir.part("equal_to_level")[0]
    got, _ = one(raw)
    assert not got["balanced"] and got["dropped"] > 0 and not sp.directed_edges_balanced(raw["triangles"])
    axes = [np.linspace(-1, 1, n).astype(F) for n in ir.NOISE_SHAPE]
    field = np.random.default_rng(3).integers(-1, 2, ir.NOISE_SHAPE).astype(F) * F(0.5) + F(0.25)
    capped = sr.extract_surface(cc.clean(field[None], 0.25, close_border=True)["sigma_out"], axes, 0.25)
    got, _ = one(capped)
    by_index = sp.directed_edges_balanced(capped["triangles"])
    print(f"capped lattice with a third on the level: by value {got}, balanced by index {by_index}")
    assert got["balanced"] and got["dropped"] > 0 and got["vertices"] < len(capped["vertices"]) and ir.directed_edges_balanced(capped)
    assert by_index                                                     # (recorded: see the docstring and DESIGN.md 24)
    mesh = ar.duplicated_tetrahedron()
    got, _ = one(mesh)
    assert got["closed_manifold"] and (got["vertices"], got["edges"], got["candidates"], got["euler_characteristic"]) == (4, 6, 4, 2)
    assert not sp.directed_edges_balanced(mesh["triangles"]) and ir.directed_edges_balanced(mesh)
    assert got["signed_volume"] == pytest.approx(1 / 6, abs=1e-15) and got["area"] == pytest.approx(1.5 + 0.75 ** 0.5, abs=1e-15)


def test_reference_on_the_off_lattice_simplification_with_and_without_duplicates():
    field, axes = sr.sphere_field(33)
    fine = sr.extract_surface(field[None], axes, 0.0)
    kept = sp.simplify_mesh(fine, *ir.OFF_LATTICE, keep_duplicates=True)
    removed = sp.simplify_mesh(fine, *ir.OFF_LATTICE)
    got_kept, _ = one(kept)
    got_removed, _ = one(removed)
    assert got_kept["balanced"] and got_kept["candidates"] == len(kept["triangles"]) == 792
    assert len(removed["triangles"]) == 784 and got_removed["candidates"] == 784 and not got_removed["balanced"]
    assert got_kept["non_manifold_edges"] > 0 and not got_kept["closed_manifold"]       # two sheets of the surface meet in a cell
    print("off-lattice, kept:", got_kept, "removed:", got_removed)


@pytest.mark.parametrize("kind", ir.MESHES)
def test_reference_balance_agrees_with_the_inside_reference(kind):
    for groups in (1, 3):
        mesh, _ = ir.mesh_case(kind, groups)
        r = ar.audit(mesh)
        each = [ir.directed_edges_balanced(ir.pack([{"vertices": v, "triangles": t}])) for v, t in ar.group_slices(mesh)]
        assert [bool(c == 0) for c in r["counts"][:, 4]] == each, (kind, groups)
        assert ir.directed_edges_balanced(mesh) == all(each)
        assert each[0] or kind not in ir.BALANCED                      # (simplified_removed lost no duplicate at two steps: also balanced)
        # the candidates are pr_inside_query's
        for (v, t), got in zip(ar.group_slices(mesh), r["counts"]):
            assert int(ir.candidates(v, t)[0].sum()) == got[0] and got[0] + got[1] == len(t)


def test_reference_on_the_hand_made_hostile_mesh():
    mesh, expected = ar.hand_made()
    got, r = one(mesh)
    assert {k: got[k] for k in expected} == expected
    assert r["labels"].tolist() == [0] * 7 + [-1, -1, 0] + [-1] * 7
    cand = ir.candidates(mesh["vertices"], mesh["triangles"])[0]
    assert np.array_equal(cand, r["labels"] >= 0) and not ir.directed_edges_balanced(mesh)
    # the tetrahedron alone: closed; area and volume of the unit corner tetrahedron (the reversed copy cancels one of the two extras)
    tetra = dict(mesh, triangles=mesh["triangles"][:4], triangle_offsets=np.array([0, 4], dtype=np.int32))
    alone, _ = one(tetra)
    assert alone["closed_manifold"] and alone["euler_characteristic"] == 2 and alone["signed_volume"] == pytest.approx(1 / 6, abs=1e-15)
    assert got["signed_volume"] == pytest.approx(1 / 6, abs=1e-15)      # (+2 -1 copies of a triangle through the origin: volume term 0)
    # hostile offsets: clamped, and the rows that no group owns keep -1
    packed = ir.pack([mesh, mesh])
    packed["triangle_offsets"] = np.array([5, 3, 2 ** 31 - 1], dtype=np.int32)
    packed["vertex_offsets"] = np.array([-7, 10, 9], dtype=np.int32)
    r = ar.audit(packed)
    assert r["counts"][0].tolist() == [0] * 12 and (r["labels"][:5] == -1).all() and r["counts"][1, 0] + r["counts"][1, 1] == 2 * 17 - 5

"""Welding and compaction without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_mesh_weld (symbols, struct size, a C99
client, every refusal through both entry points, the largest accepted totals, the workspace formula), the Python argument errors, and
the properties of the numpy restatement the GPU tests compare against (tests/weld_reference.py): the recorded sizes of the sphere, the
lattice with a third of its entries on the level (both modes), the duplicated tetrahedron and the hand-made hostile mesh, and on every
mesh kind of ``inside_reference.MESHES`` that the output's audit is the input's, that identity by index is identity by value on the
output, that welding is idempotent, and that the counts are the audit's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, surface
from tests import audit_reference as ar
from tests import inside_reference as ir
from tests import weld_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
POINTERS = ("vertices", "normals", "attributes", "triangles", "vertex_offsets", "triangle_offsets", "out_vertices", "out_normals",
            "out_attributes", "out_triangles", "vertex_map", "triangle_map", "counts", "out_vertex_offsets", "out_triangle_offsets")


def valid_struct(groups=2, V=1000, T=2000, A=7):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.MeshWeld()
    s.groups, s.total_vertices, s.total_triangles, s.attribute_width = groups, V, T, A
    s.max_vertices, s.max_triangles = V, T
    for name in POINTERS:
        setattr(s, name, 256)
    return s


def both_entry_points(lib, s):
    """(status, message) of the host-only entry point and of the call with a NULL workspace, which the call refuses last."""
    size = C.c_size_t(12345)
    first = lib.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)), lib.pr_last_error()
    second = lib.pr_mesh_weld(C.byref(s), None, 0, None), lib.pr_last_error()
    return first, second, size.value


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    for name in ("pr_mesh_weld", "pr_mesh_weld_workspace_size"):
        assert getattr(built_library, name) is not None and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_mesh_weld_t" in header and "sizeof(pr_mesh_weld_t) = 152" in header
    assert "#define PR_WELD_COMPACT_ONLY 1u" in header and _lib.WELD_COMPACT_ONLY == 1 and _lib.WELD_COUNTS == wr.COUNTS == 8
    # eight 32-bit words | six input pointers | nine output pointers
    M = _lib.MeshWeld
    assert C.sizeof(M) == 32 + 6 * 8 + 9 * 8 == 152
    assert (M.vertices.offset, M.out_vertices.offset, M.counts.offset, M.out_triangle_offsets.offset) == (32, 80, 128, 144)
    assert [name for name, _ in M._fields_] == ["groups", "total_vertices", "total_triangles", "flags", "attribute_width", "max_vertices",
                                                "max_triangles", "reserved_"] + list(POINTERS)
    # the neighbours and the ABI are as they were
    assert (C.sizeof(_lib.MeshAudit), C.sizeof(_lib.Inside), C.sizeof(_lib.Closest), C.sizeof(_lib.Raycast), C.sizeof(_lib.Simplify)) == \
        (72, 136, 152, 160, 160)
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
    pr_mesh_weld_t s;
    size_t bytes = 0;
    memset(&s, 0, sizeof s);
    s.flags = PR_WELD_COMPACT_ONLY;
    if (pr_mesh_weld_workspace_size(&s, &bytes) == 0) return 1;         /* a zeroed description is refused */
    if (pr_mesh_weld(&s, NULL, 0, NULL) == 0) return 2;
    printf("sizeof(pr_mesh_weld_t) %zu, flags at %zu, attribute_width at %zu, vertices at %zu, triangle_offsets at %zu, out_vertices at "
           "%zu, triangle_map at %zu, counts at %zu, out_triangle_offsets at %zu, refusal: %s\n", sizeof(pr_mesh_weld_t),
           offsetof(pr_mesh_weld_t, flags), offsetof(pr_mesh_weld_t, attribute_width), offsetof(pr_mesh_weld_t, vertices),
           offsetof(pr_mesh_weld_t, triangle_offsets), offsetof(pr_mesh_weld_t, out_vertices), offsetof(pr_mesh_weld_t, triangle_map),
           offsetof(pr_mesh_weld_t, counts), offsetof(pr_mesh_weld_t, out_triangle_offsets), pr_last_error());
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
    M = _lib.MeshWeld
    assert (f"sizeof(pr_mesh_weld_t) {C.sizeof(M)}, flags at {M.flags.offset}, attribute_width at {M.attribute_width.offset}, vertices at "
            f"{M.vertices.offset}, triangle_offsets at {M.triangle_offsets.offset}, out_vertices at {M.out_vertices.offset}, triangle_map at "
            f"{M.triangle_map.offset}, counts at {M.counts.offset}, out_triangle_offsets at {M.out_triangle_offsets.offset},") in run.stdout


def _break(**fields):
    def edit(s):
        for field, value in fields.items():
            setattr(s, field, value)
    return edit


REFUSALS = [
    ("null_vertices", _break(vertices=None), b"NULL vertices"),
    ("null_triangles", _break(triangles=None), b"NULL triangles"),
    ("null_vertex_offsets", _break(vertex_offsets=None), b"NULL offsets"),
    ("null_triangle_offsets", _break(triangle_offsets=None), b"NULL offsets"),
    ("null_out_vertex_offsets", _break(out_vertex_offsets=None), b"NULL offsets (out_"),
    ("null_out_triangle_offsets", _break(out_triangle_offsets=None), b"NULL offsets (out_"),
    ("null_counts", _break(counts=None), b"NULL counts"),
    ("no_groups", _break(groups=0), b"groups 0"),
    ("negative_groups", _break(groups=-2), b"groups -2"),
    ("negative_vertex_total", _break(total_vertices=-1), b"negative total"),
    ("negative_triangle_total", _break(total_triangles=-1), b"negative total"),
    ("negative_vertex_capacity", _break(max_vertices=-1), b"negative capacity"),
    ("negative_triangle_capacity", _break(max_triangles=-1), b"negative capacity"),
    ("flag_bit_1", _break(flags=2), b"unknown flag bits 0x2"),
    ("flag_bit_31", _break(flags=0x80000001), b"unknown flag bits 0x80000001"),
    ("negative_attribute_width", _break(attribute_width=-1), b"attribute_width -1"),
    ("attribute_width_too_large", _break(attribute_width=4097), b"attribute_width 4097"),
    ("out_attributes_without_attributes", _break(attributes=None), b"out_attributes needs attributes"),
    ("out_attributes_without_width", _break(attribute_width=0), b"out_attributes needs attributes"),
    ("out_normals_without_normals", _break(normals=None), b"out_normals without normals"),
    ("out_normals_without_out_vertices", _break(out_vertices=None, out_attributes=None), b"without out_vertices"),
    ("out_attributes_without_out_vertices", _break(out_vertices=None, out_normals=None), b"without out_vertices"),
    ("vertex_total_too_large", _break(total_vertices=2 ** 30), b"below 2^31"),
    ("triangle_total_too_large", _break(total_triangles=2 ** 31 - 512), b"below 2^31"),
    ("too_many_groups", _break(groups=2 ** 23), b"below 2^31"),
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


def test_optional_pointers_and_the_flag_are_accepted(built_library):
    for edit in (_break(flags=1), _break(attribute_width=4096), _break(attribute_width=0, out_attributes=None),
                 _break(attributes=None, out_attributes=None), _break(normals=None, out_normals=None),
                 _break(out_vertices=None, out_normals=None, out_attributes=None), _break(vertex_map=None, triangle_map=None),
                 _break(out_vertices=None, out_normals=None, out_attributes=None, out_triangles=None, vertex_map=None, triangle_map=None),
                 _break(max_vertices=0, max_triangles=0), _break(reserved_=77)):
        s = valid_struct()
        edit(s)
        first, second, _ = both_entry_points(built_library, s)
        assert first[0] == 0 and second[0] == PR_ERR_INVALID and b"NULL workspace" in second[1], (first, second)


def test_the_call_alone_refuses_the_workspace(built_library):
    lib = built_library
    s = valid_struct()
    size = C.c_size_t()
    assert lib.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)) == 0
    assert lib.pr_mesh_weld_workspace_size(C.byref(s), None) == PR_ERR_INVALID and b"NULL bytes" in lib.pr_last_error()
    assert lib.pr_mesh_weld_workspace_size(None, C.byref(size)) == PR_ERR_INVALID and lib.pr_mesh_weld(None, None, 0, None) == PR_ERR_INVALID
    assert lib.pr_mesh_weld(C.byref(s), None, size.value, None) == PR_ERR_INVALID and b"NULL workspace" in lib.pr_last_error()
    assert lib.pr_mesh_weld(C.byref(s), 256 + 8, size.value, None) == PR_ERR_INVALID and b"256-byte aligned" in lib.pr_last_error()
    assert lib.pr_mesh_weld(C.byref(s), 256, size.value - 1, None) == PR_ERR_INVALID and b"workspace too small" in lib.pr_last_error()
    # the workspace is refused LAST: a broken description with a broken workspace names the description
    s.counts = None
    assert lib.pr_mesh_weld(C.byref(s), 256 + 8, 0, None) == PR_ERR_INVALID and b"NULL counts" in lib.pr_last_error()


def test_the_largest_totals_are_accepted_and_the_next_are_not(built_library):
    """2 V + 256 G and T + 256 G stay below 2^31.  The call itself is asked with a NULL workspace, which it refuses last: that
    message says the description passed."""
    lib = built_library
    largest_v, largest_t = (2 ** 31 - 256 - 1) // 2, 2 ** 31 - 256 - 1
    assert 2 * largest_v + 256 < 2 ** 31 <= 2 * (largest_v + 1) + 256 and largest_t + 256 < 2 ** 31 <= largest_t + 1 + 256
    s = valid_struct(groups=1, V=largest_v, T=largest_t, A=4096)
    first, second, size = both_entry_points(lib, s)
    assert first[0] == 0 and second[0] == PR_ERR_INVALID and b"NULL workspace" in second[1], (first, second)
    assert size > 20 * largest_v + 4 * largest_t
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
    want = (4 * up(4 * (G + 1)) + up(8 * V) + 3 * up(4 * V) + up(4 * T) + up(4 * BV) + up(4 * (BV + 1)) + up(4 * BT) + up(4 * (BT + 1)) +
            up(12 * BV))
    size = C.c_size_t()
    s = valid_struct(G, V, T)
    assert built_library.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want
    s.flags, s.attribute_width = 1, 0                                   # (neither the mode nor the outputs asked for change it)
    for name in POINTERS[6:12] + ("normals", "attributes"):
        setattr(s, name, None)
    assert built_library.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    mesh = surface.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32))
    for call in (lambda: surface.weld_meshes([mesh]), lambda: surface.weld_meshes([mesh], merge=False, maps=True), lambda: mesh.welded(),
                 lambda: mesh.welded(maps=True), lambda: mesh.compacted(), lambda: mesh.keep_shells(1, compact=True),
                 lambda: surface.extract_surface(torch.zeros(1, 2, 2, 2), [torch.zeros(2)] * 3, 0.5, weld=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="at least one mesh"):
        surface.weld_meshes([])
    with pytest.raises(TypeError):
        surface.weld_meshes([mesh], False)                              # merge and maps are keywords
    with pytest.raises(TypeError):
        mesh.compacted(maps=True)
    for n in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="integer >= 1"):
            mesh.keep_shells(n, compact=True)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    s = surface.weld_struct(torch.zeros(3, 3), z(1, 3), z(3), z(3), 3, 1, z(2, 8), z(3), z(3))
    assert (s.groups, s.total_vertices, s.total_triangles, s.flags, s.attribute_width, s.max_vertices, s.max_triangles) == (2, 3, 1, 0, 0, 0, 0)
    assert (s.normals, s.attributes, s.out_vertices, s.out_normals, s.out_attributes, s.out_triangles, s.vertex_map, s.triangle_map) == (None,) * 8
    s = surface.weld_struct(torch.zeros(3, 3), z(1, 3), z(3), z(3), 3, 1, z(2, 8), z(3), z(3), attributes=torch.zeros(3, 5),
                            out_vertices=torch.zeros(2, 3), out_attributes=torch.zeros(2, 5), out_triangles=z(4, 3), merge=False)
    assert (s.flags, s.attribute_width, s.max_vertices, s.max_triangles) == (_lib.WELD_COMPACT_ONLY, 5, 2, 4)
    import inspect
    for f in (surface.extract_surface, surface.Mesh.keep_shells):
        assert inspect.signature(f).parameters["weld" if f is surface.extract_surface else "compact"].default is False
    from playableenvironments_amd import ObjectComposer
    assert inspect.signature(ObjectComposer.extract_mesh).parameters["weld"].default is False
    assert "welded mesh" in surface.RayGrid.contains.__doc__ and "welded mesh" in surface.Mesh.audit.__doc__


# ------------------------------------------------------------------------------------------------ the reference's own properties
def sizes(mesh, merge=True):
    """``(V_in, V_out, T_in, T_out, counts[2:6])`` of a single-group mesh, and the result."""
    r = wr.weld(mesh, merge)
    c = r["counts"][0].tolist()
    assert len(r["vertices"]) == c[0] and len(r["triangles"]) == c[1] and c[6:] == [0, 0]
    return (len(mesh["vertices"]), c[0], len(mesh["triangles"]), c[1], c[2:6]), r


def test_reference_gives_the_recorded_sizes():
    sphere = ir.part("sphere")[0]
    got, r = sizes(sphere)
    assert got == (1418, 1418, 2832, 2832, [0, 0, 0, 0])
    # nothing to do: the output is the input bit for bit and the maps are the identity
    assert np.array_equal(r["vertices"].view(np.uint32), sphere["vertices"].astype(F).view(np.uint32))
    assert np.array_equal(r["triangles"], sphere["triangles"]) and r["triangles"].dtype == np.int32
    assert np.array_equal(r["vertex_map"], np.arange(1418)) and np.array_equal(r["triangle_map"], np.arange(2832))
    level = ir.part("equal_to_level")[0]
    assert sizes(level)[0] == (13855, 8689, 26486, 21864, [4622, 0, 5166, 0])
    assert sizes(level, merge=False)[0] == (13855, 13686, 26486, 21864, [4622, 0, 0, 169])
    assert sizes(ar.duplicated_tetrahedron())[0] == (12, 4, 4, 4, [0, 0, 8, 0])
    got, r = sizes(ar.hand_made()[0])
    assert got == (10, 4, 17, 8, [9, 3, 2, 1])
    # by hand: classes {0, 4}, {1, 5}, 2, 3 stay; 6..8 are not finite; 9 is referenced by a dropped triangle only
    assert r["vertex_map"].tolist() == [0, 1, 2, 3, 0, 1, -1, -1, -1, -1]
    assert r["triangle_map"].tolist() == [0, 1, 2, 3, 4, 5, 6, -1, -1, 7] + [-1] * 7
    assert r["triangles"].tolist() == [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 1, 3], [3, 1, 0], [2, 1, 1]]
    got, r = sizes(ar.hand_made()[0], merge=False)
    # compact-only: 4 and 5 stay vertices of their own (triangles 3 and 9 refer to them); the kept triangles are the same
    assert got == (10, 6, 17, 8, [9, 3, 0, 1]) and r["vertex_map"].tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1, -1]
    assert r["triangles"].tolist()[3] == [4, 3, 2] and r["triangles"].tolist()[7] == [2, 5, 1]


def test_reference_carries_the_representatives_rows_bit_for_bit():
    mesh = ar.hand_made()[0]
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, (10, 5), dtype=np.uint64).astype(np.uint32)
    bits[0, 0], bits[1, 1] = 0x7FC00001, 0xFFC12345                     # NaNs with payloads
    normals = rng.integers(0, 2 ** 32, (10, 3), dtype=np.uint64).astype(np.uint32)
    r = wr.weld(mesh, True, normals=normals.view(F), attributes=bits.view(F))
    assert np.array_equal(r["attributes"].view(np.uint32), bits[:4]) and np.array_equal(r["normals"].view(np.uint32), normals[:4])
    r = wr.weld(mesh, False, attributes=bits.view(F))
    assert np.array_equal(r["attributes"].view(np.uint32), bits[:6]) and r["normals"] is None


@pytest.mark.parametrize("groups", (1, 3))
@pytest.mark.parametrize("kind", ir.MESHES)
def test_reference_output_is_an_audit_equal_index_identified_fixed_point(kind, groups):
    mesh, _ = ir.mesh_case(kind, groups)
    before = ar.audit(mesh)
    for merge in (True, False):
        r = wr.weld(mesh, merge)
        after = ar.audit(r)
        # the audit of the output is the input's, except that nothing is dropped
        want = before["counts"].copy()
        want[:, 1] = 0
        assert np.array_equal(after["counts"], want), (kind, groups, merge)
        sizes_in = np.diff(mesh["vertex_offsets"])
        assert np.array_equal(sizes_in, r["counts"][:, 0] + r["counts"][:, 3] + r["counts"][:, 4] + r["counts"][:, 5])
        assert np.array_equal(r["counts"][:, 1] + r["counts"][:, 2], np.diff(mesh["triangle_offsets"]))
        assert np.array_equal(r["counts"][:, 1:3], before["counts"][:, 0:2])
        if merge:
            assert np.array_equal(r["counts"][:, 0], before["counts"][:, 2])
            for vertices, _ in ar.group_slices(r):                     # classes by index are classes by value
                assert np.array_equal(ar.representatives(vertices), np.arange(len(vertices)))
        else:
            assert not r["counts"][:, 4].any()
        again = wr.weld(r, merge)                                       # idempotent
        for key in ("vertices", "triangles", "vertex_offsets", "triangle_offsets"):
            assert np.array_equal(again[key].view(np.uint32) if key == "vertices" else again[key], r[key].view(np.uint32) if key == "vertices" else r[key])
        assert np.array_equal(again["vertex_map"], np.concatenate([np.arange(n) for n in r["counts"][:, 0]]))
        assert not again["counts"][:, 2:].any()
        # the measures: the same candidates with the same coordinates, in the same order - the plain float64 sums are equal
        assert np.array_equal(after["measures"], before["measures"])


def test_reference_clamps_hostile_offsets_and_leaves_unowned_rows_alone():
    mesh = ar.hand_made()[0]
    packed = ir.pack([mesh, mesh])
    packed["triangle_offsets"] = np.array([5, 3, 2 ** 31 - 1], dtype=np.int32)
    packed["vertex_offsets"] = np.array([-7, 10, 9], dtype=np.int32)
    r = wr.weld(packed)
    assert r["counts"][0].tolist() == [0, 0, 0, 3, 2, 5, 0, 0]           # group 0: ten vertices, no triangle
    assert (r["triangle_map"][:5] == -1).all() and (r["vertex_map"][:10] == -1).all()
    assert r["counts"][1].tolist() == [0, 0, 2 * 17 - 5, 0, 0, 0, 0, 0]   # group 1: no vertex, so every triangle is dropped
    assert (r["triangle_map"][5:] == -1).all() and (r["vertex_map"][10:] == -1).all()
    assert r["vertex_offsets"].tolist() == [0, 0, 0] and r["triangle_offsets"].tolist() == [0, 0, 0]
    # offsets that arrive late: the first five rows of either kind belong to nobody
    packed["vertex_offsets"], packed["triangle_offsets"] = np.array([5, 10, 20], dtype=np.int32), np.array([5, 17, 34], dtype=np.int32)
    r = wr.weld(packed)
    assert (r["vertex_map"][:5] == -1).all() and (r["triangle_map"][:5] == -1).all()
    assert np.array_equal(r["counts"][1], wr.weld(mesh)["counts"][0]) and r["counts"][0, 0] + r["counts"][0, 3:6].sum() == 5

"""Mesh extraction without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_extract_surface (symbols, struct size, every
refusal, the workspace sum), the properties of the numpy reference the GPU tests compare against (tests/surface_reference.py), and
the host side of ``surface.Mesh``."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, surface
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1


def valid_struct(groups=2, points=(5, 6, 7)):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.Surface()
    s.groups = groups
    for a in range(3):
        s.points[a] = points[a]
        s.axis[a] = 256
    s.level = 0.5
    s.sigma = 256
    s.vertex_offsets = 256
    s.triangle_offsets = 256
    return s


def round256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    assert built_library.pr_surface_workspace_size is not None and built_library.pr_extract_surface is not None
    assert {"pr_surface_workspace_size", "pr_extract_surface"} <= set(_lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_surface_t" in header
    # int32 groups, int32 points[3], float level, uint32 flags | sigma, axis[3] | two int32 capacities | five pointers
    assert C.sizeof(_lib.Surface) == 4 + 12 + 4 + 4 + 8 + 24 + 4 + 4 + 5 * 8 == 104


def test_plain_c_client_sees_the_same_struct(built_library, tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    source = tmp_path / "client.c"
    source.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "playrender.h"
int main(void) {
    pr_surface_t s;
    size_t bytes = 0;
    memset(&s, 0, sizeof s);
    if (pr_surface_workspace_size(&s, &bytes) == 0) return 1;          /* a zeroed description is refused */
    if (pr_extract_surface(&s, NULL, 0, NULL) == 0) return 2;
    printf("sizeof(pr_surface_t) %zu, refusal: %s\n", sizeof(pr_surface_t), pr_last_error());
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
    assert f"sizeof(pr_surface_t) {C.sizeof(_lib.Surface)}," in run.stdout


def _break(field, value):
    def edit(s):
        setattr(s, field, value)
    return edit


def _break_index(field, index, value):
    def edit(s):
        getattr(s, field)[index] = value
    return edit


REFUSALS = [
    ("null_sigma", _break("sigma", None), b"NULL sigma"),
    ("null_axis", _break_index("axis", 1, None), b"NULL axis"),
    ("null_vertex_offsets", _break("vertex_offsets", None), b"NULL offsets"),
    ("null_triangle_offsets", _break("triangle_offsets", None), b"NULL offsets"),
    ("no_groups", _break("groups", 0), b"groups 0"),
    ("one_point", _break_index("points", 2, 1), b"points[2] = 1"),
    ("nan_level", _break("level", float("nan")), b"level is NaN"),
    ("flags", _break("flags", 4), b"flags 0x4"),
    ("negative_vertices", _break("max_vertices", -1), b"negative capacity"),
    ("negative_triangles", _break("max_triangles", -1), b"negative capacity"),
    ("normals_alone", _break("normals", 256), b"normals need vertices"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_device_work(built_library, name, edit, message):
    """Each broken description is refused by both entry points with PR_ERR_INVALID and its message; the pointers are dummies, so a
    call that got past the checks would not survive."""
    lib = built_library
    s = valid_struct()
    edit(s)
    size = C.c_size_t()
    assert lib.pr_surface_workspace_size(C.byref(s), C.byref(size)) == PR_ERR_INVALID
    assert message in lib.pr_last_error(), lib.pr_last_error()
    assert lib.pr_extract_surface(C.byref(s), 256, 1 << 40, None) == PR_ERR_INVALID
    assert message in lib.pr_last_error(), lib.pr_last_error()


def test_refuses_lattices_whose_counts_leave_int32(built_library):
    lib = built_library
    size = C.c_size_t()
    s = valid_struct(groups=1, points=(564, 564, 563))
    assert 12 * 564 * 564 * 563 >= 2 ** 31
    assert lib.pr_surface_workspace_size(C.byref(s), C.byref(size)) == PR_ERR_INVALID
    assert b"below 2^31" in lib.pr_last_error()
    assert lib.pr_extract_surface(C.byref(s), 256, 1 << 40, None) == PR_ERR_INVALID
    s = valid_struct(groups=1, points=(564, 564, 562))         # the largest accepted depth of that footprint
    assert 12 * 564 * 564 * 562 < 2 ** 31
    assert lib.pr_surface_workspace_size(C.byref(s), C.byref(size)) == 0
    s = valid_struct(groups=3, points=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))
    assert lib.pr_surface_workspace_size(C.byref(s), C.byref(size)) == PR_ERR_INVALID


def test_refuses_bad_workspaces(built_library):
    lib = built_library
    s = valid_struct()
    size = C.c_size_t()
    assert lib.pr_surface_workspace_size(C.byref(s), C.byref(size)) == 0
    assert lib.pr_extract_surface(C.byref(s), 256 + 64, size.value, None) == PR_ERR_INVALID
    assert b"256-byte aligned" in lib.pr_last_error()
    assert lib.pr_extract_surface(C.byref(s), 256, size.value - 1, None) == PR_ERR_INVALID
    assert b"workspace too small" in lib.pr_last_error()
    assert lib.pr_extract_surface(C.byref(s), None, size.value, None) == PR_ERR_INVALID


@pytest.mark.parametrize("groups,points", [(1, (2, 2, 2)), (2, (5, 6, 7)), (3, (16, 16, 17)), (1, (128, 128, 128)), (5, (9, 17, 33))])
def test_workspace_size_is_the_documented_sum(built_library, groups, points):
    """include/playrender.h: G P + G P + 4 G P + 4 x 4 G B + 8 bytes, every region rounded up to 256, B = ceil(P / 256)."""
    s = valid_struct(groups, points)
    size = C.c_size_t()
    assert built_library.pr_surface_workspace_size(C.byref(s), C.byref(size)) == 0
    P = points[0] * points[1] * points[2]
    B = (P + 255) // 256
    assert size.value == 2 * round256(groups * P) + round256(4 * groups * P) + 4 * round256(4 * groups * B) + round256(8)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        surface.extract_surface(torch.zeros(1, 4, 4, 4), [torch.arange(4.0)] * 3, 0.0)


# ------------------------------------------------------------------------------------------------ the reference's own properties
@pytest.fixture(scope="module")
def closed_meshes():
    out = {}
    for name, (field, axes) in (("sphere17", sr.sphere_field(17)), ("sphere33", sr.sphere_field(33)), ("torus33", sr.torus_field(33))):
        out[name] = sr.extract_surface(field[None], axes, 0.0)
    return out


@pytest.mark.parametrize("name,V,T,euler", [("sphere17", 1418, 2832, 2), ("sphere33", 5786, 11568, 2), ("torus33", 5540, 11080, 0)])
def test_reference_meshes_are_closed_oriented_manifolds(closed_meshes, name, V, T, euler):
    m = closed_meshes[name]
    assert (len(m["vertices"]), len(m["triangles"])) == (V, T)
    assert m["vertex_offsets"].tolist() == [0, V] and m["triangle_offsets"].tolist() == [0, T]
    assert sr.directed_edges_once(m["triangles"])             # every directed edge once, its reverse once
    assert sr.euler_characteristic(V, m["triangles"]) == euler
    assert sr.signed_volume(m["vertices"], m["triangles"]) > 0
    assert sr.triangle_areas(m["vertices"], m["triangles"]).min() > 0


def test_reference_sphere_volume_area_and_normals(closed_meshes):
    m = closed_meshes["sphere33"]
    r = 0.63
    volume = sr.signed_volume(m["vertices"], m["triangles"]) / (4 / 3 * math.pi * r ** 3) - 1
    area = sr.triangle_areas(m["vertices"], m["triangles"]).sum() / (4 * math.pi * r * r) - 1
    print(f"sphere, 33 points: volume error {volume:+.4%}, area error {area:+.4%}")
    assert abs(volume) < 0.01 and abs(area) < 0.01
    for name in ("sphere17", "sphere33"):
        v = closed_meshes[name]["vertices"].astype(np.float64)
        worst = np.abs(closed_meshes[name]["normals"] - v / np.linalg.norm(v, axis=1, keepdims=True)).max()
        print(f"{name}: worst normal component error {worst:.2e}")
        assert worst < 1e-5            # central differences are exact on a quadratic field


def test_reference_plane_on_non_uniform_axes():
    field, axes = sr.plane_field()
    m = sr.extract_surface(field[None], axes, 1.4)
    v = m["vertices"].astype(np.float64)
    assert (len(v), len(m["triangles"])) == (109, 180)
    residual = np.abs(0.3 * v[:, 0] - 0.2 * v[:, 1] + 0.5 * v[:, 2] - 1.4).max()
    print(f"plane: worst residual {residual:.2e}")
    assert residual < 1e-6
    assert (sr.triangle_normals(m["vertices"], m["triangles"]) @ np.array([0.3, -0.2, 0.5]) < 0).all()


def test_reference_table_covers_every_case_with_matching_faces():
    """16 rows per tetrahedron; 0 / 1 / 2 triangles by the number of inside corners; every entry is a crossing edge of the case."""
    count, lower, direction, corner = sr.lookup_tables()
    for t in range(6):
        rows = sr.case_rows(sr.PERMUTATIONS[t])
        assert len(rows) == 16
        for mask, triangles in enumerate(rows):
            inside = bin(mask).count("1")
            assert len(triangles) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside] == count[t, mask]
            for tri in triangles:
                assert len(set(tri)) == 3
                for i, j in tri:
                    assert i < j and (mask >> i & 1) != (mask >> j & 1)


# ------------------------------------------------------------------------------------------------ Mesh (host side)
def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        parts = line.split()
        if not parts or parts[0].startswith("#"):
            continue
        if parts[0] == "v":
            v.append([float(x) for x in parts[1:]])
        elif parts[0] == "vn":
            vn.append([float(x) for x in parts[1:]])
        elif parts[0] == "f":
            corners = [p.split("/") for p in parts[1:]]
            for c in corners:
                assert len(c) == 1 or (len(c) == 3 and c[1] == "" and c[2] == c[0])
            f.append([int(c[0]) - 1 for c in corners])
    return v, vn, f


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_obj_round_trips(tmp_path, with_normals):
    field, axes = sr.sphere_field(9)
    m = sr.extract_surface(field[None], axes, 0.0)
    mesh = Mesh(torch.from_numpy(m["vertices"]), torch.from_numpy(m["triangles"]), torch.from_numpy(m["normals"]) if with_normals else None)
    path = tmp_path / "mesh.obj"
    mesh.save_obj(path)
    v, vn, f = _parse_obj(path)
    assert torch.equal(torch.tensor(v, dtype=torch.float32), mesh.vertices)               # (%.9g round-trips fp32)
    assert torch.equal(torch.tensor(f, dtype=torch.int32), mesh.triangles)
    if with_normals:
        assert torch.equal(torch.tensor(vn, dtype=torch.float32), mesh.normals)
    else:
        assert vn == []


def test_transformed_applies_rotation_and_translation():
    field, axes = sr.sphere_field(9)
    m = sr.extract_surface(field[None], axes, 0.0)
    mesh = Mesh(torch.from_numpy(m["vertices"]), torch.from_numpy(m["triangles"]), torch.from_numpy(m["normals"]),
                torch.arange(len(m["vertices"]) * 2, dtype=torch.float32).reshape(-1, 2))
    a = 0.7
    matrix = torch.tensor([[math.cos(a), -math.sin(a), 0, 1.0], [math.sin(a), math.cos(a), 0, -2.0], [0, 0, 1, 0.5], [0, 0, 0, 1]])
    world = mesh.transformed(matrix)
    x, y, z = mesh.vertices.double().unbind(-1)
    want = torch.stack([math.cos(a) * x - math.sin(a) * y + 1.0, math.sin(a) * x + math.cos(a) * y - 2.0, z + 0.5], -1)
    assert torch.allclose(world.vertices.double(), want, rtol=1e-6, atol=1e-6)
    nx, ny, nz = mesh.normals.double().unbind(-1)
    want_n = torch.stack([math.cos(a) * nx - math.sin(a) * ny, math.sin(a) * nx + math.cos(a) * ny, nz], -1)
    assert torch.allclose(world.normals.double(), want_n, rtol=1e-6, atol=1e-6)
    assert world.triangles is mesh.triangles and world.features is mesh.features
    assert torch.equal(mesh.vertices, torch.from_numpy(m["vertices"]))                    # the original is untouched
    # orientation survives a rigid motion
    assert sr.signed_volume(world.vertices.numpy(), world.triangles.numpy()) > 0
    with pytest.raises(ValueError):
        mesh.transformed(torch.eye(3))

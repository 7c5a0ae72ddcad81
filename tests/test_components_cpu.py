"""Component labelling without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_label_components (symbols, struct size,
every refusal, the workspace sum), the Python argument errors, and the properties of the numpy reference the GPU tests compare
against (tests/components_reference.py): adjacency, the two-blob scene, floater removal and capping seen through the reference
mesher (tests/surface_reference.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, clean_lattice, label_components, surface
from tests import components_reference as cr
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1


def valid_struct(groups=2, points=(5, 6, 7), sigma_out=False):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    c = _lib.Components()
    c.groups = groups
    for a in range(3):
        c.points[a] = points[a]
    c.level = 0.5
    c.fill = 0.5
    c.sigma = 1 << 20
    c.counts = 256
    if sigma_out:
        c.sigma_out = 1 << 30
    return c


def round256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    assert built_library.pr_components_workspace_size is not None and built_library.pr_label_components is not None
    assert {"pr_components_workspace_size", "pr_label_components"} <= set(_lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_components_t" in header and "#define PR_ABI_VERSION 5" in header
    assert "#define PR_COMPONENTS_CLOSE_BORDER 1u" in header and "#define PR_COMPONENTS_MAX_KEEP 8" in header
    assert (_lib.COMPONENTS_CLOSE_BORDER, _lib.COMPONENTS_MAX_KEEP) == (1, 8)
    # int32 groups, int32 points[3] | float level, uint32 flags | two int32 | float fill, uint32 reserved | five pointers
    assert C.sizeof(_lib.Components) == 4 + 12 + 4 + 4 + 4 + 4 + 4 + 4 + 5 * 8 == 80


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
    pr_components_t c;
    size_t bytes = 0;
    memset(&c, 0, sizeof c);
    if (pr_components_workspace_size(&c, &bytes) == 0) return 1;       /* a zeroed description is refused */
    if (pr_label_components(&c, NULL, 0, NULL) == 0) return 2;
    printf("sizeof(pr_components_t) %zu, flag %u, cap %d, refusal: %s\n", sizeof(pr_components_t), PR_COMPONENTS_CLOSE_BORDER,
           PR_COMPONENTS_MAX_KEEP, pr_last_error());
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
    assert f"sizeof(pr_components_t) {C.sizeof(_lib.Components)}, flag 1, cap 8," in run.stdout


def _break(field, value):
    def edit(c):
        setattr(c, field, value)
    return edit


def _break_index(field, index, value):
    def edit(c):
        getattr(c, field)[index] = value
    return edit


def _overlap(offset):
    def edit(c):
        c.sigma_out = c.sigma + offset
    return edit


LATTICE_BYTES = 2 * 5 * 6 * 7 * 4
REFUSALS = [
    ("null_sigma", _break("sigma", None), b"NULL sigma"),
    ("null_counts", _break("counts", None), b"NULL counts"),
    ("no_groups", _break("groups", 0), b"groups 0"),
    ("negative_groups", _break("groups", -3), b"groups -3"),
    ("no_points", _break_index("points", 1, 0), b"points[1] = 0"),
    ("nan_level", _break("level", float("nan")), b"level is NaN"),
    ("unknown_flag", _break("flags", 2), b"flags 0x2"),
    ("unknown_flag_beside_the_known", _break("flags", 5), b"flags 0x5"),
    ("keep_largest_9", _break("keep_largest", 9), b"keep_largest 9"),
    ("keep_largest_negative", _break("keep_largest", -1), b"keep_largest -1"),
    ("min_points_negative", _break("min_points", -1), b"min_points -1"),
    ("fill_above_level", _break("fill", 0.75), b"fill 0.75 must be <= level"),
    ("fill_nan", _break("fill", float("nan")), b"must be <= level"),
    ("overlap_behind", _overlap(4), b"overlaps sigma partially"),
    ("overlap_last_value", _overlap(LATTICE_BYTES - 4), b"overlaps sigma partially"),
    ("overlap_in_front", _overlap(-(LATTICE_BYTES - 4)), b"overlaps sigma partially"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_device_work(built_library, name, edit, message):
    """Each broken description is refused by both entry points with PR_ERR_INVALID and its message; the pointers are dummies, so a
    call that got past the checks would not survive."""
    lib = built_library
    c = valid_struct(sigma_out=True)
    edit(c)
    size = C.c_size_t()
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == PR_ERR_INVALID
    assert message in lib.pr_last_error(), lib.pr_last_error()
    assert lib.pr_label_components(C.byref(c), 256, 1 << 40, None) == PR_ERR_INVALID
    assert message in lib.pr_last_error(), lib.pr_last_error()


def test_accepted_descriptions(built_library):
    """What must NOT be refused: the fill is not looked at without sigma_out, in place and adjacent buffers, every legal selection."""
    lib = built_library
    size = C.c_size_t()
    c = valid_struct()
    c.fill = float("nan")
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0, lib.pr_last_error()
    for offset in (0, LATTICE_BYTES, -LATTICE_BYTES):
        c = valid_struct(sigma_out=True)
        c.sigma_out = c.sigma + offset
        assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0, (offset, lib.pr_last_error())
    c = valid_struct(sigma_out=True)
    c.flags, c.keep_largest, c.min_points, c.fill = 1, 8, 2 ** 31 - 1, float("-inf")
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0, lib.pr_last_error()
    assert lib.pr_components_workspace_size(C.byref(c), None) == PR_ERR_INVALID


def test_refuses_lattices_whose_indices_leave_int32(built_library):
    lib = built_library
    size = C.c_size_t()
    c = valid_struct(groups=2, points=(1024, 1024, 1024))
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == PR_ERR_INVALID
    assert b"below 2^31" in lib.pr_last_error()
    assert lib.pr_label_components(C.byref(c), 256, 1 << 40, None) == PR_ERR_INVALID
    c = valid_struct(groups=1, points=(2 ** 31 - 1, 1, 1))          # the largest accepted lattice
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0
    c = valid_struct(groups=3, points=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == PR_ERR_INVALID


def test_refuses_bad_workspaces(built_library):
    lib = built_library
    c = valid_struct()
    size = C.c_size_t()
    assert lib.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0
    assert lib.pr_label_components(C.byref(c), 256 + 64, size.value, None) == PR_ERR_INVALID
    assert b"256-byte aligned" in lib.pr_last_error()
    assert lib.pr_label_components(C.byref(c), 256, size.value - 1, None) == PR_ERR_INVALID
    assert b"workspace too small" in lib.pr_last_error()
    assert lib.pr_label_components(C.byref(c), None, size.value, None) == PR_ERR_INVALID
    assert b"NULL workspace" in lib.pr_last_error()


@pytest.mark.parametrize("groups,points", [(1, (1, 1, 1)), (2, (5, 6, 7)), (3, (16, 16, 17)), (1, (128, 128, 128))])
def test_workspace_size_is_the_documented_sum(built_library, groups, points):
    """include/playrender.h: 4 G P + 4 G P + 64 G bytes, every region rounded up to 256."""
    size = C.c_size_t()
    for keep in (0, 8):                          # (the selection does not change the size)
        c = valid_struct(groups, points)
        c.keep_largest = keep
        assert built_library.pr_components_workspace_size(C.byref(c), C.byref(size)) == 0
        P = points[0] * points[1] * points[2]
        assert size.value == 2 * round256(4 * groups * P) + round256(64 * groups)


def test_python_argument_errors():
    cpu = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_components(cpu, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clean_lattice(cpu, 0.0, keep_largest=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        surface.extract_surface(cpu, [torch.arange(4.0)] * 3, 0.0, keep_largest=1, close_border=True)
    for bad in (dict(keep_largest=9), dict(keep_largest=-1), dict(min_points=-1), dict(fill=0.5), dict(fill=float("nan"))):
        with pytest.raises(ValueError):
            clean_lattice(cpu, 0.0, **bad)
    with pytest.raises(TypeError):
        clean_lattice(cpu, 0.0, 1)                                   # the selection is keyword-only
    with pytest.raises(TypeError):
        label_components(cpu, 0.0, True)
    assert surface.label_components is label_components and surface.clean_lattice is clean_lattice


# ------------------------------------------------------------------------------------------------ the reference's own properties
def test_reference_adjacency_is_the_seven_directions_and_not_their_mirror_images():
    f = np.zeros((1, 3, 3, 3), dtype=np.float32)
    for at in ((0, 0, 0), (1, 1, 0), (2, 0, 2), (1, 1, 2)):
        f[0][at] = 1.0
    labels, sizes = cr.label_components(f, 0.5)
    assert cr.components_of(labels, sizes) == [[(0, 2), (14, 1), (20, 1)]]      # (0,0,0)-(1,1,0) is an edge, (2,0,2)-(1,1,2) is not
    assert labels[0][1, 1, 0] == 0 and labels[0][1, 1, 2] == 14 and labels[0][2, 0, 2] == 20 and labels[0][0, 0, 1] == -1
    assert sizes[0][0, 0, 0] == sizes[0][1, 1, 0] == 2 and sizes[0][0, 0, 1] == 0
    for d in cr.DIRECTIONS:                     # every direction joins, its mirror image along x does not (unless it is one of the seven)
        for sign in (1, -1):
            g = np.zeros((1, 3, 3, 3), dtype=np.float32)
            g[0][1, 1, 1] = g[0][1 + sign * d[0], 1 + sign * d[1], 1 + sign * d[2]] = 1.0
            assert cr.clean(g, 0.5)["counts"].tolist() == [[2, 1, 1, 2]]
        mirrored = (-d[0], d[1], d[2])
        if d[0] and (d[1] or d[2]):
            g = np.zeros((1, 3, 3, 3), dtype=np.float32)
            g[0][1, 1, 1] = g[0][1 + mirrored[0], 1 + mirrored[1], 1 + mirrored[2]] = 1.0
            assert cr.clean(g, 0.5)["counts"].tolist() == [[2, 2, 2, 2]]


def test_reference_inside_rule_and_bitwise_copies():
    f = np.array([[[[np.nan, 0.5, 0.75], [np.inf, -np.inf, 0.25]]]], dtype=np.float32)
    f.view(np.int32)[0, 0, 0, 0] = 0x7FC12345                      # a NaN with a payload
    out = cr.clean(f, 0.5, min_points=2, fill=-1.0)
    assert out["labels"].reshape(-1).tolist() == [-1, -1, 2, 3, -1, -1]                # NaN and the level itself are outside
    assert out["counts"].tolist() == [[2, 2, 0, 0]]
    want = [0x7FC12345] + cr.bits(np.array([0.5, -1, -1, -np.inf, 0.25], dtype=np.float32)).tolist()      # both singles blanked
    assert cr.bits(out["sigma_out"]).reshape(-1).tolist() == want


def test_reference_selection_ranks_by_size_then_label():
    ranked = [(40, 5), (3, 5), (17, 9), (90, 1), (60, 1)]
    ranked = sorted(ranked, key=lambda c: (-c[1], c[0]))
    assert ranked == [(17, 9), (3, 5), (40, 5), (60, 1), (90, 1)]
    assert cr.kept_labels(ranked) == [17, 3, 40, 60, 90]
    assert cr.kept_labels(ranked, keep_largest=2) == [17, 3]                           # the tie goes to the smaller label
    assert cr.kept_labels(ranked, min_points=5) == [17, 3, 40]
    assert cr.kept_labels(ranked, min_points=6, keep_largest=2) == [17]                # rank counts every component
    assert cr.kept_labels(ranked, keep_largest=8) == [17, 3, 40, 60, 90]


@pytest.fixture(scope="module")
def blobs():
    return {n: cr.two_blob_field(n) for n in (17, 33)}


@pytest.mark.parametrize("n,sizes,closed", [(17, [268, 17, 2, 1, 1, 1], [268, 17, 1, 1, 1, 1]), (33, [2120, 140, 2, 1, 1, 1], [2120, 140, 1, 1, 1, 1])])
def test_reference_two_blob_scene(blobs, n, sizes, closed):
    field, _ = blobs[n]
    for close_border, want in ((False, sizes), (True, closed)):
        out = cr.clean(field[None], 0.0, close_border=close_border)
        ranked = cr.components_of(out["labels"], out["sizes"])[0]
        assert [size for _, size in ranked] == want
        assert out["counts"].tolist() == [[sum(want), 6, 6, sum(want)]]
        assert np.array_equal(cr.bits(out["sigma_out"]) != cr.bits(field[None]), cr.inside_mask(field[None], 0.0) & (out["labels"] < 0))
    labels = cr.clean(field[None], 0.0)["labels"][0]
    assert labels[n - 2, 1, 2] != labels[n - 3, 2, 3]               # the pair along (-1, 1, 1) is no edge
    assert labels[2, n - 1, 2] == labels[1, n - 2, 1] == (n + n - 2) * n + 1       # the pair along (1, 1, 1) is


@pytest.mark.parametrize("n,V,T,V0,T0", [(17, 890, 1776, 1090, 2152), (33, 3552, 7100, 4184, 8340)])
def test_reference_keeping_the_largest_component_leaves_its_mesh_alone(blobs, n, V, T, V0, T0):
    field, axes = blobs[n]
    out = cr.clean(field[None], 0.0, keep_largest=1)
    assert out["counts"][0, 2] == 1 and out["counts"][0, 3] == out["sizes"].max()
    before = sr.extract_surface(field[None], axes, 0.0)
    after = sr.extract_surface(out["sigma_out"], axes, 0.0)
    assert (len(before["vertices"]), len(before["triangles"])) == (V0, T0)
    assert (len(after["vertices"]), len(after["triangles"])) == (V, T)
    assert sr.directed_edges_once(after["triangles"]) and sr.euler_characteristic(V, after["triangles"]) == 2
    rows = {row.tobytes() for row in before["vertices"]}
    assert all(row.tobytes() in rows for row in after["vertices"])     # no vertex of the kept component moved


def test_reference_capping_closes_a_surface_that_leaves_the_lattice():
    field, axes = sr.sphere_field(17, r=1.2)
    open_mesh = sr.extract_surface(field[None], axes, 0.0)
    assert (len(open_mesh["vertices"]), len(open_mesh["triangles"])) == (2798, 5160)
    assert not sr.directed_edges_once(open_mesh["triangles"])
    out = cr.clean(field[None], 0.0, close_border=True, fill=0.0)
    capped = sr.extract_surface(out["sigma_out"], axes, 0.0)
    assert (len(capped["vertices"]), len(capped["triangles"])) == (4490, 8976)
    assert sr.directed_edges_once(capped["triangles"]) and sr.euler_characteristic(4490, capped["triangles"]) == 2
    assert not np.isnan(capped["vertices"]).any() and not np.isnan(capped["normals"]).any()
    assert sr.triangle_areas(capped["vertices"], capped["triangles"]).min() == 0        # fill == level: zero-area triangles, kept

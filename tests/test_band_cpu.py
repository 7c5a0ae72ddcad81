"""Band evaluation without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_band_plan / pr_band_fill (symbols, struct size,
every refusal, the workspace sum), the Python argument errors, and the properties of the numpy reference the GPU tests compare
against (tests/band_reference.py): the skeleton, the fill, and - through the reference mesher (tests/surface_reference.py) - that with
one guard cell the band lattice of a surface the skeleton sees gives the dense lattice's mesh, normals included."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, surface
from tests import band_reference as br
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1


def valid_struct(groups=2, points=(5, 6, 7), stride=2, guard=1):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    b = _lib.Band()
    b.groups = groups
    for a in range(3):
        b.points[a] = points[a]
        b.axis[a] = 4096 + 256 * a
    b.level = 0.5
    b.stride = stride
    b.guard = guard
    b.sigma = 1 << 20
    b.point_offsets = 256
    b.counts = 512
    return b


def round256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    for name in ("pr_band_workspace_size", "pr_band_plan", "pr_band_fill"):
        assert getattr(built_library, name) is not None and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_band_t" in header and "#define PR_ABI_VERSION 5" in header
    assert "#define PR_BAND_MIN_STRIDE 2" in header and "#define PR_BAND_MAX_STRIDE 64" in header and "#define PR_BAND_MAX_GUARD 8" in header
    assert (_lib.BAND_MIN_STRIDE, _lib.BAND_MAX_STRIDE, _lib.BAND_MAX_GUARD) == (2, 64, 8)
    # int32 groups, int32 points[3] | float level, uint32 flags | int32 stride, guard | int32 max_points, uint32 reserved | 11 pointers
    assert C.sizeof(_lib.Band) == 4 + 12 + 4 + 4 + 4 + 4 + 4 + 4 + 11 * 8 == 128
    assert built_library.pr_abi_version() == 5


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
    pr_band_t b;
    size_t bytes = 0;
    memset(&b, 0, sizeof b);
    if (pr_band_workspace_size(&b, &bytes) == 0) return 1;       /* a zeroed description is refused */
    if (pr_band_plan(&b, NULL, 0, NULL) == 0) return 2;
    if (pr_band_fill(&b, NULL, 0, NULL) == 0) return 3;
    printf("sizeof(pr_band_t) %zu, strides %d..%d, guard %d, refusal: %s\n", sizeof(pr_band_t), PR_BAND_MIN_STRIDE, PR_BAND_MAX_STRIDE,
           PR_BAND_MAX_GUARD, pr_last_error());
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
    assert f"sizeof(pr_band_t) {C.sizeof(_lib.Band)}, strides 2..64, guard 8," in run.stdout


def _break(field, value):
    def edit(b):
        setattr(b, field, value)
    return edit


def _break_index(field, index, value):
    def edit(b):
        getattr(b, field)[index] = value
    return edit


REFUSALS = [
    ("null_sigma", _break("sigma", None), b"NULL sigma"),
    ("null_axis", _break_index("axis", 1, None), b"NULL axis"),
    ("null_point_offsets", _break("point_offsets", None), b"NULL point_offsets"),
    ("null_counts", _break("counts", None), b"NULL counts"),
    ("no_groups", _break("groups", 0), b"groups 0"),
    ("negative_groups", _break("groups", -3), b"groups -3"),
    ("one_point", _break_index("points", 1, 1), b"points[1] = 1"),
    ("no_points", _break_index("points", 2, 0), b"points[2] = 0"),
    ("stride_1", _break("stride", 1), b"stride 1"),
    ("stride_0", _break("stride", 0), b"stride 0"),
    ("stride_65", _break("stride", 65), b"stride 65"),
    ("guard_negative", _break("guard", -1), b"guard -1"),
    ("guard_9", _break("guard", 9), b"guard 9"),
    ("nan_level", _break("level", float("nan")), b"level is NaN"),
    ("flags", _break("flags", 1), b"flags 0x1"),
    ("negative_capacity", _break("max_points", -1), b"negative capacity"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_device_work(built_library, name, edit, message):
    """Each broken description is refused by all three entry points with PR_ERR_INVALID and its message; the pointers are dummies, so
    a call that got past the checks would not survive."""
    lib = built_library
    b = valid_struct()
    edit(b)
    size = C.c_size_t()
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == PR_ERR_INVALID
    assert message in lib.pr_last_error(), lib.pr_last_error()
    for call in (lib.pr_band_plan, lib.pr_band_fill):
        assert call(C.byref(b), 256, 1 << 40, None) == PR_ERR_INVALID
        assert message in lib.pr_last_error(), lib.pr_last_error()


def test_fill_refuses_missing_values(built_library):
    b = valid_struct()
    b.max_points = 3
    size = C.c_size_t()
    assert built_library.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0
    assert built_library.pr_band_fill(C.byref(b), 256, size.value, None) == PR_ERR_INVALID
    assert b"NULL values" in built_library.pr_last_error()


def test_accepted_descriptions(built_library):
    lib = built_library
    size = C.c_size_t()
    for stride, guard, points in ((2, 0, (2, 2, 2)), (64, 8, (2, 2, 2)), (64, 8, (300, 2, 5)), (7, 3, (30, 33, 35))):
        b = valid_struct(points=points, stride=stride, guard=guard)
        assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0, lib.pr_last_error()
    b = valid_struct()
    b.level = float("inf")
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0, lib.pr_last_error()
    assert lib.pr_band_workspace_size(C.byref(b), None) == PR_ERR_INVALID
    assert lib.pr_band_workspace_size(None, C.byref(size)) == PR_ERR_INVALID


def test_refuses_lattices_whose_indices_leave_int32(built_library):
    lib = built_library
    size = C.c_size_t()
    b = valid_struct(groups=2, points=(1024, 1024, 1024))
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == PR_ERR_INVALID
    assert b"below 2^31" in lib.pr_last_error()
    assert lib.pr_band_plan(C.byref(b), 256, 1 << 40, None) == PR_ERR_INVALID
    assert lib.pr_band_fill(C.byref(b), 256, 1 << 40, None) == PR_ERR_INVALID
    b = valid_struct(groups=1, points=(2 ** 29 - 1, 2, 2))          # just below
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0
    b = valid_struct(groups=1, points=(2 ** 29, 2, 2))
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == PR_ERR_INVALID
    b = valid_struct(groups=3, points=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == PR_ERR_INVALID


def test_refuses_bad_workspaces(built_library):
    lib = built_library
    b = valid_struct()
    size = C.c_size_t()
    assert lib.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0
    for call in (lib.pr_band_plan, lib.pr_band_fill):
        assert call(C.byref(b), 256 + 64, size.value, None) == PR_ERR_INVALID
        assert b"256-byte aligned" in lib.pr_last_error()
        assert call(C.byref(b), 256, size.value - 1, None) == PR_ERR_INVALID
        assert b"workspace too small" in lib.pr_last_error()
        assert call(C.byref(b), None, size.value, None) == PR_ERR_INVALID
        assert b"NULL workspace" in lib.pr_last_error()


@pytest.mark.parametrize("groups,points,stride", [(1, (2, 2, 2), 2), (2, (5, 6, 7), 2), (3, (16, 16, 17), 3), (1, (128, 128, 128), 4),
                                                  (2, (30, 33, 35), 7), (1, (9, 17, 33), 64)])
def test_workspace_size_is_the_documented_sum(built_library, groups, points, stride):
    """include/playrender.h: G C + G C + 2 x 4 G D + 2 x 4 G B + 4 bytes, every region rounded up to 256."""
    size = C.c_size_t()
    for guard in (0, 8):                         # (the guard does not change the size)
        b = valid_struct(groups, points, stride, guard)
        assert built_library.pr_band_workspace_size(C.byref(b), C.byref(size)) == 0
        P = points[0] * points[1] * points[2]
        cells = [len(br.skeleton_indices(n, stride)) - 1 for n in points]
        assert cells == [-(-(n - 1) // stride) for n in points]
        Cc = cells[0] * cells[1] * cells[2]
        B, D = -(-P // 256), -(-Cc // 256)
        assert size.value == 2 * round256(groups * Cc) + 2 * round256(4 * groups * D) + 2 * round256(4 * groups * B) + 256


def test_python_argument_errors():
    cpu = torch.zeros(1, 4, 4, 4)
    axes = [torch.arange(4.0)] * 3
    nothing = lambda g, positions: positions[:, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        surface.refine_band(cpu, axes, 0.0, stride=2, evaluate=nothing)
    with pytest.raises(TypeError):
        surface.refine_band(cpu, axes, 0.0, 2, 1, nothing)              # stride, guard and evaluate are keyword-only
    with pytest.raises(TypeError):
        surface.refine_band(cpu, axes, 0.0, evaluate=nothing)           # ... and the stride has no default
    for bad in (0, 1, 65, -2):
        with pytest.raises(ValueError, match="stride"):
            surface.skeleton_indices(9, bad)
    with pytest.raises(ValueError):
        surface.skeleton_indices(1, 2)


# ------------------------------------------------------------------------------------------------ the reference's own properties
@pytest.mark.parametrize("n,stride,want", [(2, 2, [0, 1]), (2, 64, [0, 1]), (9, 4, [0, 4, 8]), (10, 4, [0, 4, 8, 9]), (7, 3, [0, 3, 6]),
                                           (8, 3, [0, 3, 6, 7]), (33, 64, [0, 32]), (5, 2, [0, 2, 4])])
def test_skeleton_indices(n, stride, want):
    assert surface.skeleton_indices(n, stride) == want == br.skeleton_indices(n, stride).tolist()
    lo, hi, idx = br.cell_ranges(n, stride)
    assert idx.tolist() == want and lo[0] == hi[0] == 0 and lo[-1] == hi[-1] == len(want) - 2
    for i in range(n):                           # an inner skeleton index lies in two cells, every other index in one
        assert hi[i] - lo[i] == (1 if i in want[1:-1] else 0)


def test_reference_on_a_hand_made_lattice():
    """(5, 5, 9), stride 4: cells (1, 1, 2); one inside corner at (0, 0, 0): only the first cell is mixed."""
    f = np.full((1, 5, 5, 9), np.nan, dtype=np.float32)
    f[0][np.ix_([0, 4], [0, 4], [0, 4, 8])] = -1.0
    f[0, 0, 0, 0] = 1.0
    p = br.plan(f, 0.0, 4, 0)
    assert p["cells"] == (1, 1, 2) and p["mixed"].reshape(-1).tolist() == [1, 0] == p["active"].reshape(-1).tolist()
    band = p["band"][0]
    assert band[:, :, :5].sum() == 5 * 5 * 5 - 8 and band[:, :, 5:].sum() == 0          # the shared face k = 4 belongs to the active cell
    assert p["counts"].tolist() == [[2, 1, 1, 117]] and p["point_offsets"].tolist() == [0, 117]
    assert p["point_index"][:3].tolist() == [1, 2, 3] and np.all(np.diff(p["point_index"]) > 0)
    out, exact = br.fill(f, p, np.arange(117, dtype=np.float32), 4)
    assert exact.sum() == 117 + 12 and out.view(np.float32)[0, 0, 0, 1] == 0.0 and out.view(np.float32)[0, 4, 4, 3] == 116.0
    assert np.all(out.view(np.float32)[0, :, :, 5:8] == -1.0)                          # copies of the corner (0, 0, 4)
    assert np.array_equal(out[0][np.ix_([0, 4], [0, 4], [0, 4, 8])], br.bits(f)[0][np.ix_([0, 4], [0, 4], [0, 4, 8])])
    assert br.plan(f, 0.0, 4, 1)["counts"].tolist() == [[2, 1, 2, 5 * 5 * 9 - 12]]      # one guard cell: everything


def test_reference_copies_bits():
    f = np.full((1, 3, 3, 5), 7.0, dtype=np.float32)
    f.view(np.int32)[0, 0, 0, 0] = 0x7FC12345                      # a NaN (with a payload) and -inf at skeleton corners are outside:
    f[0, 0, 0, 2] = -np.inf                                        # both cells along z are mixed
    out, exact, p = br.refine(f, 0.0, 2, 0)
    assert p["counts"].tolist() == [[2, 2, 2, 3 * 3 * 5 - 12]]
    g = np.full((1, 3, 3, 5), np.float32(-2.0))
    g.view(np.int32)[0, 0, 0, 0] = 0x7FC12345
    out, exact, p = br.refine(g, 0.0, 2, 0)
    assert p["counts"].tolist() == [[2, 0, 0, 0]] and exact.sum() == 2 * 2 * 3
    assert out.view(np.int32)[0, 0, 1, 1] == 0x7FC12345 and out.view(np.int32)[0, 1, 1, 1] == 0x7FC12345 and out[0, 1, 1, 3] == -2.0


def lattice_axes(shape):
    """Non-uniform, increasing coordinates spanning [-1, 1] on every axis."""
    rng = np.random.default_rng(100)
    axes = []
    for n in shape:
        x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n - 1))])
        axes.append((2 * x / x[-1] - 1).astype(np.float32))
    return axes


def analytic_field(kind, axes):
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in axes], indexing="ij")
    if kind == "sphere":
        return (0.63 ** 2 - X * X - Y * Y - Z * Z).astype(np.float32)
    if kind == "torus":
        return (0.23 ** 2 - (np.sqrt(X * X + Y * Y) - 0.55) ** 2 - Z * Z).astype(np.float32)
    if kind == "plane":
        return (0.3 * X - 0.2 * Y + 0.5 * Z - 0.1).astype(np.float32)
    raise KeyError(kind)


SURFACES = [("sphere", (33, 33, 33)), ("sphere", (30, 33, 35)), ("torus", (33, 33, 33)), ("torus", (30, 33, 35)), ("plane", (9, 17, 33))]
_DENSE = {}


def dense_case(kind, shape):
    """(field (1, ...), axes, the dense lattice's reference mesh, the stencil support of its crossing edges); computed once."""
    if (kind, shape) not in _DENSE:
        axes = lattice_axes(shape)
        field = analytic_field(kind, axes)[None]
        ends = br.crossing_ends(field[0], 0.0)
        _DENSE[(kind, shape)] = (field, axes, sr.extract_surface(field, axes, 0.0), ends, br.gradient_stencil(ends))
    return _DENSE[(kind, shape)]


@pytest.mark.parametrize("stride", [2, 3, 4])
@pytest.mark.parametrize("kind,shape", SURFACES, ids=[f"{k}_{'x'.join(map(str, s))}" for k, s in SURFACES])
def test_one_guard_cell_keeps_the_mesh(kind, shape, stride):
    """guard = 1: every end of a crossing edge and every point of its gradient stencil is exact, so the mesh of the band lattice is the
    dense lattice's in vertices, triangles and normals - at a fraction of the points."""
    field, axes, want, ends, stencil = dense_case(kind, shape)
    lattice, exact, p = br.refine(field, 0.0, stride, 1)
    assert ends.sum() > 0 and int((ends & (exact[0] == 0)).sum()) == 0 and int((stencil & (exact[0] == 0)).sum()) == 0
    assert np.array_equal(br.bits(lattice)[exact == 1], br.bits(field)[exact == 1])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(lattice > 0, field > 0)                  # the copies are on the right side everywhere
    got = sr.extract_surface(lattice, axes, 0.0)
    for key in ("vertex_offsets", "triangle_offsets", "vertices", "triangles", "normals"):
        assert np.array_equal(got[key], want[key]), key
    share = float(exact.mean())
    print(f"{kind} {shape} stride {stride}: {p['counts'].tolist()}, {share:.3f} of the points evaluated")
    assert share < 1.0


def test_without_a_guard_cell_the_mesh_differs():
    """guard = 0 is not enough: on the 33^3 sphere at stride 3 points of the gradient stencil (on other axes: ends of crossing edges
    too) lie in no mixed cell, and the mesh is not the dense lattice's.  Equality is claimed for guard >= 1 only."""
    field, axes, want, ends, stencil = dense_case("sphere", (33, 33, 33))
    lattice, exact, _ = br.refine(field, 0.0, 3, 0)
    missed = int((stencil & (exact[0] == 0)).sum())
    print(f"guard 0: {int((ends & (exact[0] == 0)).sum())} edge ends and {missed} stencil points are not exact")
    assert missed > 0
    got = sr.extract_surface(lattice, axes, 0.0)
    same = all(got[key].shape == want[key].shape and np.array_equal(got[key], want[key]) for key in ("vertices", "triangles", "normals"))
    assert not same

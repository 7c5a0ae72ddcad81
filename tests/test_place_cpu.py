"""Quadric placement without a GPU (python -m pytest tests -m "not gpu"): the C ABI of pr_mesh_place (symbols, struct size and field
offsets, every refusal through both entry points, the largest accepted totals, the workspace formula), the Python argument errors, the
unit's resource report (no scratch), and the properties of the numpy restatement the GPU tests compare against
(tests/place_reference.py) on the boxes, the rotated box and the spheres of DESIGN.md 29: what the placement is for - the volume that
the mean rule loses comes back - and what it must not do."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, surface
from tests import place_reference as pl
from tests import simplify_reference as sp
from tests import surface_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_ERR_INVALID = -1
F = np.float32
WORDS = ("groups", "total_vertices", "total_triangles", "flags", "total_merged_vertices", "total_merged_triangles", "scale",
         "regularisation", "max_move", "reserved_")
POINTERS = ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "vertex_map", "merged_vertices", "merged_vertex_offsets",
            "merged_triangles", "merged_triangle_offsets", "out_vertices", "counts")
BOX_VOLUME = 8 * 0.53 * 0.41 * 0.37
SPHERE_VOLUME = 4 / 3 * np.pi * 0.63 ** 3


def valid_struct(groups=2, V=1000, T=2000, VO=300, TO=600):
    """A description with non-NULL dummy pointers: enough for the host-only checks (nothing is launched before they pass)."""
    s = _lib.MeshPlace()
    s.groups, s.total_vertices, s.total_triangles, s.flags, s.total_merged_vertices, s.total_merged_triangles = groups, V, T, 0, VO, TO
    s.scale, s.regularisation = 0.125, 2.0 ** -10
    for a in range(3):
        s.max_move[a] = 0.125
    for i, name in enumerate(POINTERS):
        setattr(s, name, 256 * (i + 1))
    return s


def both_entry_points(lib, s):
    """(status, message) of the host-only entry point and of the call with a NULL workspace, which the call refuses last."""
    size = C.c_size_t(12345)
    first = lib.pr_mesh_place_workspace_size(C.byref(s), C.byref(size)), lib.pr_last_error()
    second = lib.pr_mesh_place(C.byref(s), None, 0, None), lib.pr_last_error()
    return first, second, size.value


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_and_struct_size(built_library):
    for name in ("pr_mesh_place", "pr_mesh_place_workspace_size"):
        assert getattr(built_library, name) is not None and name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    assert "typedef struct pr_mesh_place_t" in header and "sizeof(pr_mesh_place_t) = 136" in header
    # twelve 32-bit words | nine input pointers | two output pointers
    M = _lib.MeshPlace
    assert C.sizeof(M) == 48 + 9 * 8 + 2 * 8 == 136 and _lib.PLACE_COUNTS == pl.COUNTS == 4
    assert [getattr(M, name).offset for name in WORDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 44]
    assert [getattr(M, name).offset for name in POINTERS] == [48 + 8 * i for i in range(11)]
    assert [name for name, _ in M._fields_] == list(WORDS) + list(POINTERS)
    # the neighbours and the ABI are as they were
    assert (C.sizeof(_lib.Simplify), C.sizeof(_lib.MeshSmooth), C.sizeof(_lib.MeshWeld)) == (160, 120, 152)
    assert built_library.pr_abi_version() == 5 and "#define PR_ABI_VERSION 5" in header


def _break(**fields):
    def edit(s):
        for field, value in fields.items():
            if field.startswith("max_move"):
                s.max_move[int(field[-1])] = value
            else:
                setattr(s, field, value)
    return edit


REFUSALS = [
    ("null_vertices", _break(vertices=None), b"NULL vertices"),
    ("null_triangles", _break(triangles=None), b"NULL triangles"),
    ("null_vertex_offsets", _break(vertex_offsets=None), b"NULL offsets"),
    ("null_triangle_offsets", _break(triangle_offsets=None), b"NULL offsets"),
    ("null_merged_vertex_offsets", _break(merged_vertex_offsets=None), b"NULL offsets"),
    ("null_vertex_map", _break(vertex_map=None), b"NULL vertex_map"),
    ("null_merged_vertices", _break(merged_vertices=None), b"NULL merged_vertices"),
    ("null_out_vertices", _break(out_vertices=None), b"NULL out_vertices"),
    ("null_counts", _break(counts=None), b"NULL counts"),
    ("triangles_without_offsets", _break(merged_triangle_offsets=None), b"both or neither"),
    ("offsets_without_triangles", _break(merged_triangles=None), b"both or neither"),
    ("no_groups", _break(groups=0), b"groups 0"),
    ("negative_groups", _break(groups=-2), b"groups -2"),
    ("negative_vertex_total", _break(total_vertices=-1), b"negative total"),
    ("negative_triangle_total", _break(total_triangles=-1), b"negative total"),
    ("negative_merged_vertex_total", _break(total_merged_vertices=-1), b"negative total"),
    ("negative_merged_triangle_total", _break(total_merged_triangles=-1), b"negative total"),
    ("flag_bit_0", _break(flags=1), b"unknown flag bits 0x1"),
    ("flag_bit_31", _break(flags=0x80000000), b"unknown flag bits 0x80000000"),
    ("scale_zero", _break(scale=0.0), b"scale"),
    ("scale_negative", _break(scale=-1.0), b"scale"),
    ("scale_nan", _break(scale=float("nan")), b"scale"),
    ("scale_inf", _break(scale=float("inf")), b"scale"),
    ("regularisation_zero", _break(regularisation=0.0), b"regularisation"),
    ("regularisation_negative", _break(regularisation=-0.5), b"regularisation"),
    ("regularisation_nan", _break(regularisation=float("nan")), b"regularisation"),
    ("regularisation_inf", _break(regularisation=float("inf")), b"regularisation"),
    ("max_move_negative", _break(max_move1=-0.25), b"max_move[1]"),
    ("max_move_nan", _break(max_move0=float("nan")), b"max_move[0]"),
    ("max_move_inf", _break(max_move2=float("inf")), b"max_move[2]"),
    ("out_is_vertices", _break(out_vertices=256 * 1), b"out_vertices is an input"),
    ("out_is_merged_vertices", _break(out_vertices=256 * 6), b"out_vertices is an input"),
    ("vertex_total_too_large", _break(total_vertices=2 ** 31 - 512), b"below 2^31"),
    ("triangle_total_too_large", _break(total_triangles=2 ** 31 - 512), b"below 2^31"),
    ("merged_vertex_total_too_large", _break(total_merged_vertices=2 ** 31 - 512), b"below 2^31"),
    ("merged_triangle_total_too_large", _break(total_merged_triangles=2 ** 31 - 512), b"below 2^31"),
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


def test_optional_pointers_and_the_limits_are_accepted(built_library):
    for edit in (_break(merged_triangles=None, merged_triangle_offsets=None), _break(max_move0=0.0, max_move1=0.0, max_move2=0.0),
                 _break(scale=1e-30), _break(scale=3e38, regularisation=3e38), _break(regularisation=1e-38),
                 _break(total_vertices=0, total_triangles=0, total_merged_vertices=0, total_merged_triangles=0)):
        s = valid_struct()
        edit(s)
        first, second, _ = both_entry_points(built_library, s)
        assert first[0] == 0 and second[0] == PR_ERR_INVALID and b"NULL workspace" in second[1], (first, second)


def test_the_call_alone_refuses_the_workspace_and_last(built_library):
    lib = built_library
    s = valid_struct()
    size = C.c_size_t()
    assert lib.pr_mesh_place_workspace_size(C.byref(s), C.byref(size)) == 0
    assert lib.pr_mesh_place_workspace_size(C.byref(s), None) == PR_ERR_INVALID and b"NULL bytes" in lib.pr_last_error()
    assert lib.pr_mesh_place_workspace_size(None, C.byref(size)) == PR_ERR_INVALID and lib.pr_mesh_place(None, None, 0, None) == PR_ERR_INVALID
    assert lib.pr_mesh_place(C.byref(s), None, size.value, None) == PR_ERR_INVALID and b"NULL workspace" in lib.pr_last_error()
    assert lib.pr_mesh_place(C.byref(s), 256 + 8, size.value, None) == PR_ERR_INVALID and b"256-byte aligned" in lib.pr_last_error()
    assert lib.pr_mesh_place(C.byref(s), 256, size.value - 1, None) == PR_ERR_INVALID and b"workspace too small" in lib.pr_last_error()
    s.counts = None                                                     # a broken description with a broken workspace names the description
    assert lib.pr_mesh_place(C.byref(s), 256 + 8, 0, None) == PR_ERR_INVALID and b"NULL counts" in lib.pr_last_error()


def test_the_largest_totals_are_accepted_and_the_next_are_not(built_library):
    largest = 2 ** 31 - 256 - 1
    assert largest + 256 < 2 ** 31 <= largest + 1 + 256
    fields = ("total_vertices", "total_triangles", "total_merged_vertices", "total_merged_triangles")
    for field in fields:
        s = valid_struct(groups=1)
        setattr(s, field, largest)
        first, second, size = both_entry_points(built_library, s)
        assert first[0] == 0 and second[0] == PR_ERR_INVALID and b"NULL workspace" in second[1], (field, first, second)
        assert field != "total_merged_vertices" or size > 76 * largest
        setattr(s, field, largest + 1)
        first, second, _ = both_entry_points(built_library, s)
        assert first[0] == second[0] == PR_ERR_INVALID and b"below 2^31" in first[1] and b"below 2^31" in second[1], field
    assert both_entry_points(built_library, valid_struct(groups=3, V=0, T=0, VO=0, TO=0))[0][0] == 0       # empty input is valid


@pytest.mark.parametrize("G,V,T,VO,TO", [(1, 0, 0, 0, 0), (1, 1, 1, 1, 1), (3, 1000, 2000, 300, 600), (5, 4321, 98765, 1234, 2468),
                                         (2, 256, 512, 255, 257), (64, 63, 65, 7, 9)])
def test_the_workspace_is_the_documented_sum(built_library, G, V, T, VO, TO):
    up = lambda n: (n + 255) // 256 * 256
    want = 8 * up(4 * (G + 1)) + up(72 * VO) + up(4 * VO)
    size = C.c_size_t()
    s = valid_struct(G, V, T, VO, TO)
    assert built_library.pr_mesh_place_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want
    s.merged_triangles = s.merged_triangle_offsets = None               # (neither the parameters nor the optional input change it)
    s.scale, s.regularisation = 3.0, 0.5
    assert built_library.pr_mesh_place_workspace_size(C.byref(s), C.byref(size)) == 0 and size.value == want


def test_cpu_tensors_and_bad_arguments_are_refused_by_the_python_layer():
    import inspect
    from playableenvironments_amd import ObjectComposer
    mesh = surface.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32))
    small = surface.Mesh(torch.zeros(2, 3), torch.zeros((1, 3), dtype=torch.int32))
    vmap = torch.zeros(4, dtype=torch.int32)
    grid = ([0, 0, 0], [1, 1, 1], [2, 2, 2])
    for call in (lambda: surface.place_vertices([mesh], [small], [vmap], scale=1.0, max_move=1.0),
                 lambda: surface.simplify_meshes([mesh], *grid, placement="quadric"),
                 lambda: mesh.simplified(*grid, placement="quadric"),
                 lambda: surface.extract_surface(torch.zeros(1, 2, 2, 2), [torch.zeros(2)] * 3, 0.5, simplify=2, placement="quadric")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call in (lambda: surface.simplify_meshes([mesh], *grid, placement="median"), lambda: mesh.simplified(*grid, placement=None),
                 lambda: surface.simplify_meshes([mesh], *grid, placement="Quadric")):
        with pytest.raises(ValueError, match="placement must be one of"):
            call()
    with pytest.raises(ValueError, match="at least one mesh"):
        surface.place_vertices([], [], [], scale=1.0, max_move=1.0)
    with pytest.raises(ValueError, match="one merged mesh and one vertex map per mesh"):
        surface.place_vertices([mesh], [small, small], [vmap], scale=1.0, max_move=1.0)
    with pytest.raises(ValueError, match="one entry per vertex"):
        surface.place_vertices([mesh], [small], [vmap[:3]], scale=1.0, max_move=1.0)
    with pytest.raises(TypeError):
        surface.place_vertices([mesh], [small], [vmap], 1.0, 1.0)       # everything behind the maps is a keyword
    for kw, message in ((dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
                        (dict(regularisation=0.0), "regularisation"), (dict(regularisation=float("inf")), "regularisation"),
                        (dict(max_move=-1.0), "max_move"), (dict(max_move=[1.0, 2.0]), "max_move"), (dict(max_move=[1, float("nan"), 1]), "max_move")):
        with pytest.raises(ValueError, match=message):
            surface._place_arguments(**{**dict(scale=1.0, max_move=1.0, regularisation=2.0 ** -10), **kw})
    assert surface._place_arguments(0.5, 0.25, 0.125) == (0.5, [0.25] * 3, 0.125)
    assert surface._place_arguments(2, [1, 0, 3], 1)[1] == [1.0, 0.0, 3.0]
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    s = surface.place_struct(torch.zeros(3, 3), z(1, 3), z(3), z(3), 3, 1, z(3), torch.zeros(2, 3), z(3), 2, torch.ones(2, 3), z(2, 4),
                             scale=0.25, max_move=[0.25, 0.5, 0.75])
    assert (s.groups, s.total_vertices, s.total_triangles, s.flags, s.total_merged_vertices, s.total_merged_triangles) == (2, 3, 1, 0, 2, 0)
    assert (s.scale, s.regularisation, list(s.max_move)) == (0.25, 2.0 ** -10, [0.25, 0.5, 0.75])
    assert (s.merged_triangles, s.merged_triangle_offsets) == (None, None) and None not in (s.vertex_map, s.merged_vertices, s.out_vertices)
    # "mean" is the default everywhere
    for f in (surface.simplify_meshes, surface.extract_surface, ObjectComposer.extract_mesh, surface._simplify_packed):
        assert inspect.signature(f).parameters["placement"].default == "mean"
    assert inspect.signature(surface.place_vertices).parameters["regularisation"].default == 2.0 ** -10 == surface.PLACE_REGULARISATION


def test_kernels_use_no_scratch(tmp_path):
    """The unit compiled with the Makefile's flags and the compiler's resource-usage remarks: every kernel reports 0 bytes of private
    memory per lane."""
    import re
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "playableenvironments_amd", "csrc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                          "-I", csrc, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "place.hip"), "-o",
                          str(tmp_path / "place.o")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = dict(re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", run.stderr, flags=re.S))
    kernels = {name: int(size) for name, size in usage.items() if "k_place_" in name}
    assert len(kernels) == 4 and any("k_place_accumulate" in name for name in kernels), usage
    assert all(size == 0 for size in kernels.values()), kernels


# ------------------------------------------------------------------------------------------------ the reference on hand-made input
def corner_case():
    """Three triangles in the planes x = 1, y = 1, z = 1 around the corner (1, 1, 1), none touching it; every vertex in ONE cluster."""
    v = np.array([[1, .2, .3], [1, .8, .2], [1, .4, .9], [.2, 1, .3], [.3, 1, .8], [.9, 1, .4], [.3, .2, 1], [.8, .3, 1], [.4, .9, 1]], F)
    t = np.arange(9, dtype=np.int32).reshape(3, 3)
    mean = v.astype(np.float64).mean(axis=0).astype(F)[None]
    return v, t, np.zeros(9, np.int32), mean


def test_three_planes_put_the_vertex_on_their_corner_and_max_move_holds_it():
    v, t, vmap, mean = corner_case()
    r = pl.place(v, t, [0, 9], [0, 3], vmap, mean, [0, 1], scale=1.0, max_move=[1.0] * 3)
    # (A + lambda I) y = b with A = diag(w_x, w_y, w_z), w = twice the triangle's area, lambda = regularisation (w_x + w_y + w_z) / 3:
    # axis k misses the corner by the factor lambda / (w_k + lambda) < lambda / w_k of its distance from the mean (and fp32 rounding)
    assert r["counts"].tolist() == [[1, 0, 0, 0]]
    w = pl.doubled_areas(v, t)
    allowed = 2.0 ** -10 * w.sum() / (3 * w) * np.abs(mean[0].astype(np.float64) - 1) + 2.0 ** -23
    assert (np.abs(r["vertices"][0].astype(np.float64) - 1) <= allowed).all() and allowed.max() < 1e-3
    held = pl.place(v, t, [0, 9], [0, 3], vmap, mean, [0, 1], scale=1.0, max_move=[1.0, 0.25, 1.0])     # the move is about 0.45 per axis
    assert held["counts"].tolist() == [[0, 1, 0, 0]] and np.array_equal(held["vertices"].view(np.uint32), mean.view(np.uint32))
    # a flipped triangle contributes the same quadric: the placement does not depend on the orientation
    flipped = pl.place(v, t[:, ::-1], [0, 9], [0, 3], vmap, mean, [0, 1], scale=1.0, max_move=[1.0] * 3)
    assert np.allclose(flipped["vertices"], r["vertices"], atol=1e-6)


def test_invalid_triangles_skipped_contributions_and_map_entries_out_of_range_are_counted_as_the_header_says():
    v, t, vmap, mean = corner_case()
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [.5, .5, .5]], F)])
    t = np.concatenate([t, np.array([[0, 1, 9], [0, 1, 11], [-1, 1, 2], [3, 3, 3], [0, 0, 1]], np.int32)])      # NaN, two out of range, two without area
    vmap = np.concatenate([vmap, np.zeros(2, np.int32)])
    r = pl.place(v, t, [0, 11], [0, 8], vmap, mean, [0, 1], scale=1.0, max_move=[1.0] * 3)
    clean = pl.place(v[:9], t[:3], [0, 9], [0, 3], vmap[:9], mean, [0, 1], scale=1.0, max_move=[1.0] * 3)
    assert r["counts"].tolist() == [[1, 0, 5, 0]] and np.array_equal(r["vertices"].view(np.uint32), clean["vertices"].view(np.uint32))
    # map entries outside [0, VO): the corner contributes nothing and nothing is counted; with every corner outside the vertex stays
    for entry in (-1, 1, 2 ** 31 - 1):
        out = pl.place(v[:9], t[:3], [0, 9], [0, 3], np.full(9, entry, np.int32), mean, [0, 1], scale=1.0, max_move=[1.0] * 3)
        assert out["counts"].tolist() == [[0, 1, 0, 0]] and np.array_equal(out["vertices"].view(np.uint32), mean.view(np.uint32))
    # a triangle whose corners lie in two clusters contributes once to each, one with all three in one cluster once
    two = np.concatenate([mean, mean + F(0.5)])
    sums, contributions, bad = pl.quadric_sums(v[:9], t[:3], np.array([0, 0, 1, 0, 0, 0, 1, 1, 1], np.int32), two, 1.0)
    assert contributions.tolist() == [2, 2] and bad == 0


def test_the_order_of_the_triangles_does_not_show():
    case = shared("box33_2")
    mesh, simp = case["mesh"], case["simplified"]
    order = np.random.default_rng(3).permutation(len(mesh["triangles"]))
    again = pl.place_simplified(dict(mesh, triangles=mesh["triangles"][order]), simp, case["cell"])
    assert np.array_equal(again["vertices"].view(np.uint32), case["placed"]["vertices"].view(np.uint32))
    assert np.array_equal(again["counts"], case["placed"]["counts"])


# ------------------------------------------------------------------------------------------------ the cases of DESIGN.md 29
def rotated(n):
    return pl.box_field(n, rz=0.4, rx=0.3)


CASES = {  # name: (field, lattice points, lattice steps per cell, true volume)
    "box33_2": (pl.box_field, 33, 2, BOX_VOLUME), "box33_4": (pl.box_field, 33, 4, BOX_VOLUME), "box65_4": (pl.box_field, 65, 4, BOX_VOLUME),
    "box65_8": (pl.box_field, 65, 8, BOX_VOLUME), "rotated33_2": (rotated, 33, 2, BOX_VOLUME), "rotated65_4": (rotated, 65, 4, BOX_VOLUME),
    "sphere33_2": (sr.sphere_field, 33, 2, SPHERE_VOLUME), "sphere33_4": (sr.sphere_field, 33, 4, SPHERE_VOLUME),
    "sphere65_4": (sr.sphere_field, 65, 4, SPHERE_VOLUME)}
RECORDED = {  # name: (V out, T out, turned) - DESIGN.md 29
    "box33_2": (288, 572, 0), "box33_4": (80, 156, 0), "box65_4": (288, 572, 0), "box65_8": (80, 156, 0), "rotated33_2": (380, 764, 7),
    "rotated65_4": (384, 780, 15), "sphere33_2": (488, 972, 0), "sphere33_4": (128, 252, 0), "sphere65_4": (488, 972, 0)}
_MESHES, _SHARED = {}, {}


def shared(name):
    """The fine mesh (one per field and lattice), its simplification and the placement of a case, computed once and never changed."""
    if name not in _SHARED:
        make, n, k, true_volume = CASES[name]
        if (make, n) not in _MESHES:
            field, axes = make(n)[:2]
            _MESHES[(make, n)] = (sr.extract_surface(field[None], axes, 0.0), axes)
        mesh, axes = _MESHES[(make, n)]
        origin, cell, cells = sp.lattice_grid(axes, k)
        simplified = sp.simplify_mesh(mesh, origin, cell, cells)
        _SHARED[name] = {"mesh": mesh, "simplified": simplified, "cell": cell, "placed": pl.place_simplified(mesh, simplified, cell),
                         "true_volume": true_volume}
    return _SHARED[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_what_the_placement_keeps_and_what_it_gains(name):
    case = shared(name)
    mesh, simp, placed = case["mesh"], case["simplified"], case["placed"]
    triangles, mean, quadric = simp["triangles"], simp["vertices"], placed["vertices"]
    counts = placed["counts"][0].tolist()
    error = [pl.volume(v, triangles) / case["true_volume"] - 1 for v in (mean, quadric)]
    print(f"{name}: V / T {len(mean)} / {len(triangles)}, counts {counts}, volume error {100 * error[0]:+.2f} % -> {100 * error[1]:+.2f} %")
    assert (len(mean), len(triangles), counts[3]) == RECORDED[name]
    # the triangle lists are the simplifier's: the placement returns vertices and counts only, so edge balance is what it was
    assert set(placed) == {"vertices", "counts"} and quadric.shape == mean.shape and sp.directed_edges_balanced(triangles)
    assert counts[0] == len(mean) and counts[1] == 0 and counts[2] == 0          # every cluster moved and nothing was skipped
    assert (pl.doubled_areas(quadric, triangles) > 0).all()             # no zero-area triangle
    # the turned count is what a count from the two sets of vertices gives, and 0 away from the rotated box's slivers
    before, after = sr.triangle_normals(mean, triangles), sr.triangle_normals(quadric, triangles)
    assert counts[3] == int(((before * after).sum(axis=1) < 0).sum())
    assert (counts[3] == 0) == (not name.startswith("rotated"))
    # no vertex moved further than a cell per axis
    assert (np.abs(quadric.astype(np.float64) - mean.astype(np.float64)) <= np.asarray(case["cell"])).all()
    if name.startswith("sphere"):
        assert abs(error[1]) < abs(error[0])
    else:
        assert abs(error[1]) < 0.5 * abs(error[0])
    # max_move = 0 returns the means exactly (a vertex whose three moves are exactly 0 - a flat cluster - still counts as moved)
    still = pl.place_simplified(mesh, simp, case["cell"], max_move=[0.0] * 3)
    assert np.array_equal(still["vertices"].view(np.uint32), mean.view(np.uint32)) and int(still["counts"][0, :2].sum()) == len(mean)


def test_a_cluster_without_a_contributing_triangle_keeps_its_mean():
    """Vertices that no triangle refers to are clustered like the others (the simplifier's rule); a cluster that only they reach has no
    quadric and keeps its mean bit for bit."""
    case = shared("sphere33_2")
    mesh = case["mesh"]
    lone = np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.04], [-0.9, -0.9, -0.9]], F)      # two cells that the sphere's surface does not meet
    vertices = np.concatenate([mesh["vertices"], lone])
    normals = np.concatenate([mesh["normals"], np.zeros((3, 3), F)])
    packed = dict(mesh, vertices=vertices, normals=normals, vertex_offsets=np.array([0, len(vertices)], np.int32))
    origin, cell, cells = sp.lattice_grid([np.linspace(-1, 1, 33).astype(F)] * 3, 2)
    simp = sp.simplify_mesh(packed, origin, cell, cells)
    placed = pl.place_simplified(packed, simp, cell)
    added = np.unique(simp["vertex_map"][-3:])
    assert len(added) == 2 and len(simp["vertices"]) == len(case["simplified"]["vertices"]) + 2
    assert placed["counts"][0].tolist() == [len(simp["vertices"]) - 2, 2, 0, 0]
    assert np.array_equal(placed["vertices"][added].view(np.uint32), simp["vertices"][added].view(np.uint32))
    rest = np.setdiff1d(np.arange(len(simp["vertices"])), added)
    assert np.array_equal(placed["vertices"][rest].view(np.uint32), case["placed"]["vertices"].view(np.uint32))


def test_a_planes_vertices_stay_in_the_plane_and_slide_no_further_than_the_regularisation_allows():
    """On a planar cluster the quadric is w n n^T: it says nothing about the tangent directions, and the regularisation lambda I holds
    the vertex there.  The bounds come from the input alone.  With D the largest distance of a cluster's mean from the plane of one
    of its triangles: normal to the plane the minimiser moves by a weighted mean of those distances, at most D, from a mean that lies
    within D plus the input's own deviation of the true plane; tangentially |y_t| <= |b_t| / lambda with |b_t| <= trace(A) D / h and lambda = regularisation trace(A) / 3,
    so the slide is at most 3 D / regularisation."""
    x = np.linspace(-1, 1, 17)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    field, axes, level = (0.3 * X - 0.2 * Y + 0.5 * Z).astype(F), [x.astype(F)] * 3, 0.07
    normal = np.array([0.3, -0.2, 0.5]) / np.linalg.norm([0.3, -0.2, 0.5])
    offset = level / np.linalg.norm([0.3, -0.2, 0.5])
    mesh = sr.extract_surface(field[None], axes, level)
    origin, cell, cells = sp.lattice_grid(axes, 2)
    simp = sp.simplify_mesh(mesh, origin, cell, cells)
    placed = pl.place_simplified(mesh, simp, cell)
    mean, quadric = simp["vertices"].astype(np.float64), placed["vertices"].astype(np.float64)
    assert len(mean) > 8 and placed["counts"][0, 0] == len(mean) and placed["counts"][0, 2] == 0
    off_plane = lambda p: np.abs(p @ normal - offset)
    t = mesh["triangles"].astype(np.int64)
    n = sr.triangle_normals(mesh["vertices"], t)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    D = 0.0
    for e in range(3):                                                   # the mean of a corner's cluster against the triangle's own plane
        D = max(D, float(np.abs(((mean[simp["vertex_map"][t[:, e]]] - mesh["vertices"][t[:, 0]].astype(np.float64)) * n).sum(axis=1)).max()))
    deviation = float(off_plane(mesh["vertices"].astype(np.float64)).max())
    move = quadric - mean
    slide = np.linalg.norm(move - np.outer(move @ normal, normal), axis=1).max()
    print(f"plane: {len(mean)} clusters, input off the plane by {deviation:.3g}, D {D:.3g}, output off the plane by "
          f"{off_plane(quadric).max():.3g}, largest slide {slide:.3g} (allowed {3 * D / 2.0 ** -10:.3g})")
    ulp = 2.0 ** -23 * 3.0                                              # (the output is rounded to fp32 at coordinates below 4)
    assert off_plane(quadric).max() <= deviation + 2 * D + ulp
    assert slide <= 3 * D / 2.0 ** -10 + ulp

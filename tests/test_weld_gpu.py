"""Welding and compaction on the GPU (python -m pytest tests -m gpu): ``pr_mesh_weld`` against its numpy restatement
(tests/weld_reference.py) - vertices, normals, attributes, triangles, both maps, counts and both offset arrays with ``torch.equal``, and
equal bits from call to call - through the C ABI on poisoned outputs and a poisoned workspace with guard rows behind every array; both
modes, groups at the seams of the block scan and one above 256 x 256 elements, attribute rows of random bits, counting calls and
short capacities, empty and hostile input, a recorded call replayed on another mesh, the consumers (contains, closest, cast, audit) on
the input and on the welded mesh, the Python layer, ``Mesh.keep_shells(compact=True)`` and ``ObjectComposer.extract_mesh(weld=True)``
on the small tennis networks."""
import ctypes as C

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, surface
from tests import audit_reference as ar
from tests import components_reference as cc
from tests import inside_reference as ir
from tests import surface_reference as sr
from tests import weld_reference as wr
from tests.test_raycast_gpu import device_mesh, hostile, to_meshes
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, make_field, poisoned, tennis

pytestmark = pytest.mark.gpu

F = np.float32
KERNELS = {True: 8, False: 7}      # the header's launch counts: value mode, PR_WELD_COMPACT_ONLY
MESHES = ("sphere", "torus", "plane", "noise", "equal_to_level", "capped_noise", "simplified_kept", "simplified_removed", "two_spheres",
          "duplicated_tetrahedron", "lattice_222")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes and references (numpy only), computed once
_CASES, _REFERENCES = {}, {}


def lattice_222():
    return sr.extract_surface(np.array([[[1, 0], [0, 0]], [[0, 0], [0, 1]]], dtype=F)[None], [np.array([0, 1], dtype=F)] * 3, 0.5)


def level_lattice_capped():
    """The (9, 17, 33) lattice with a third of its entries on the level, capped: closed by value, with dropped triangles."""
    axes = [np.linspace(-1, 1, n).astype(F) for n in ir.NOISE_SHAPE]
    field = np.random.default_rng(3).integers(-1, 2, ir.NOISE_SHAPE).astype(F) * F(0.5) + F(0.25)
    return ir.pack([sr.extract_surface(cc.clean(field[None], 0.25, close_border=True)["sigma_out"], axes, 0.25)]), axes


def case(kind, groups):
    """The packed mesh of one of MESHES in one group, or in three: the mesh, a sphere or torus, another of its kind."""
    key = (kind, groups)
    if key not in _CASES:
        if kind in ir.MESHES:
            mesh, _ = ir.mesh_case(kind, groups)
        else:
            first = {"two_spheres": ar.two_spheres, "duplicated_tetrahedron": ar.duplicated_tetrahedron, "lattice_222": lattice_222}[kind]()
            last = ar.two_spheres((0.27, 0.36)) if kind == "two_spheres" else first
            mesh = ir.pack([first] if groups == 1 else [first, ir.part("torus")[0], last])
        _CASES[key] = mesh
    return _CASES[key]


def random_rows(V, width, seed):
    """``(V, width)`` fp32 of random BITS: NaNs with payloads, infinities, denormals and both zeros among them."""
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, (max(V, 1), width), dtype=np.uint64).astype(np.uint32)
    bits[::7, 0] = 0x7FC00000 + np.arange(len(bits[::7]), dtype=np.uint32)       # quiet NaNs, each with its own payload
    bits[3::11, width - 1] = 0xFF800001                                            # signalling NaNs
    bits[5::13, 0] = 0x80000000                                                    # -0
    return bits[:V].view(F)


def reference(key, mesh, merge, normals=None, attributes=None, seed=0):
    """``wr.weld`` of a shared case, computed once (``key`` None: not kept)."""
    full = None if key is None else (key, merge, seed, normals is not None, None if attributes is None else attributes.shape[1])
    if full is None or full not in _REFERENCES:
        want = wr.weld(mesh, merge, normals=normals, attributes=attributes)
        if full is None:
            return want
        _REFERENCES[full] = want
    return _REFERENCES[full]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_weld(dev, totals, merge=True, normals=None, attributes=None, emit=True, maps=True, short=0, out_normals=True, out_attributes=True):
    """One call on poisoned outputs and a poisoned workspace, guard rows behind every array.  ``totals``: the output rows (vertices,
    triangles) the emitting call gets room for, minus ``short``; ``normals`` / ``attributes``: device inputs or None.  Returns the
    outputs without their guards (which are checked here) and the capacities."""
    G, V, T = dev["vertex_offsets"].numel() - 1, dev["V"], dev["T"]
    A = 0 if attributes is None else attributes.size(1)
    cap_v, cap_t = max(totals[0] - short, 0), max(totals[1] - short, 0)
    out = {"counts": poisoned((G * 8 + GUARD,), torch.int32), "out_vertex_offsets": poisoned((G + 1 + GUARD,), torch.int32),
           "out_triangle_offsets": poisoned((G + 1 + GUARD,), torch.int32)}
    rows = {"counts": G * 8, "out_vertex_offsets": G + 1, "out_triangle_offsets": G + 1}
    shapes = {"counts": (G, 8), "out_vertex_offsets": (G + 1,), "out_triangle_offsets": (G + 1,)}
    if emit:
        out["out_vertices"], rows["out_vertices"], shapes["out_vertices"] = poisoned(((cap_v + GUARD) * 3,), torch.float32), cap_v * 3, (cap_v, 3)
        out["out_triangles"], rows["out_triangles"], shapes["out_triangles"] = poisoned(((cap_t + GUARD) * 3,), torch.int32), cap_t * 3, (cap_t, 3)
        if normals is not None and out_normals:
            out["out_normals"], rows["out_normals"], shapes["out_normals"] = poisoned(((cap_v + GUARD) * 3,), torch.float32), cap_v * 3, (cap_v, 3)
        if attributes is not None and out_attributes:
            out["out_attributes"], rows["out_attributes"], shapes["out_attributes"] = poisoned(((cap_v + GUARD) * A,), torch.float32), cap_v * A, (cap_v, A)
    if maps:
        out["vertex_map"], rows["vertex_map"], shapes["vertex_map"] = poisoned((V + GUARD,), torch.int32), V, (V,)
        out["triangle_map"], rows["triangle_map"], shapes["triangle_map"] = poisoned((T + GUARD,), torch.int32), T, (T,)
    s = surface.weld_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], V, T, out["counts"],
                            out["out_vertex_offsets"], out["out_triangle_offsets"], normals=normals, attributes=attributes, merge=merge,
                            **{k: t for k, t in out.items() if k not in ("counts", "out_vertex_offsets", "out_triangle_offsets")})
    s.max_vertices, s.max_triangles = (cap_v, cap_t) if emit else (0, 0)
    size = C.c_size_t()
    lib = _lib.load()
    _lib.check(lib.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_weld_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")          # (64 guard words)
    _lib.check(lib.pr_mesh_weld(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream), "pr_mesh_weld")
    torch.cuda.synchronize()
    assert bool(is_poison(workspace[size.value // 4:]).all()), "workspace guard"
    for key, t in out.items():
        assert bool(is_poison(t[rows[key]:]).all()), ("guard", key)
    return {key: t[:rows[key]].reshape(shapes[key]) for key, t in out.items()}


REFERENCE_KEYS = {"out_vertices": "vertices", "out_normals": "normals", "out_attributes": "attributes", "out_triangles": "triangles",
                  "vertex_map": "vertex_map", "triangle_map": "triangle_map", "counts": "counts", "out_vertex_offsets": "vertex_offsets",
                  "out_triangle_offsets": "triangle_offsets"}


def assert_weld_equal(got, want, what):
    """Every output with torch.equal on its 32-bit words (floats are compared as bits: NaNs and the sign of zero count).  An output
    with fewer rows than the reference (a short capacity) holds the reference's first rows; a map with more rows than the mesh (totals
    beyond the offsets) holds -1 in the rows that no group owns."""
    for key, t in got.items():
        expected = cuda(want[REFERENCE_KEYS[key]]).view(torch.int32)
        if key in ("vertex_map", "triangle_map") and t.numel() > expected.numel():
            expected = torch.cat([expected, torch.full((t.numel() - expected.numel(),), -1, dtype=torch.int32, device="cuda")])
        if key in ("out_vertices", "out_normals", "out_attributes", "out_triangles"):
            expected = expected.reshape(-1, t.size(1))[:t.size(0)]
        assert expected.shape == t.shape, (what, key, expected.shape, t.shape)
        wrong = t.view(torch.int32) != expected
        assert not bool(wrong.any()), (what, key, int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())


def totals_of(want):
    return int(want["vertex_offsets"][-1]), int(want["triangle_offsets"][-1])


def check_case(mesh, key, merge, width=0, with_normals=False, what=None, again=True, seed=0):
    """The emitting call with both maps against the reference, and a second call into fresh buffers against the first."""
    V = len(mesh["vertices"])
    normals = random_rows(V, 3, 10 + seed) if with_normals else None
    attributes = random_rows(V, width, 20 + seed) if width else None
    want = reference(key, mesh, merge, normals, attributes, seed)
    dev = device_mesh(mesh)
    pad = lambda a: None if a is None else cuda(a if len(a) else np.zeros((1, a.shape[1]), F))
    inputs = dict(normals=pad(normals), attributes=pad(attributes))
    got = run_weld(dev, totals_of(want), merge, **inputs)
    assert_weld_equal(got, want, what or key)
    if again:
        second = run_weld(dev, totals_of(want), merge, **inputs)
        for name in got:
            assert torch.equal(got[name].view(torch.int32), second[name].view(torch.int32)), (what or key, name)
    return got, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. identity through the C ABI
@pytest.mark.parametrize("merge", [True, False], ids=["value", "compact_only"])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", MESHES)
def test_weld_equals_the_reference_and_repeats_bit_for_bit(kind, groups, merge):
    mesh = case(kind, groups)
    got, want = check_case(mesh, (kind, groups), merge, width=3, with_normals=True)
    counts = want["counts"]
    print(f"{kind} G={groups} merge={merge}: V {mesh['vertex_offsets'].tolist()} T {mesh['triangle_offsets'].tolist()} counts {counts[:, :6].tolist()}")
    assert np.array_equal(np.diff(mesh["vertex_offsets"]), counts[:, 0] + counts[:, 3] + counts[:, 4] + counts[:, 5])
    if merge:                                                           # the audit's counts [2], [0], [1]
        audit = ar.audit(mesh)["counts"]
        assert torch.equal(got["counts"][:, :3], cuda(audit[:, [2, 0, 1]]))


def test_the_recorded_answers():
    sphere = case("sphere", 1)
    got, _ = check_case(sphere, ("sphere", 1), True, again=False)
    assert got["counts"][0].tolist() == [1418, 2832, 0, 0, 0, 0, 0, 0]
    assert torch.equal(got["out_vertices"].view(torch.int32), cuda(sphere["vertices"]).view(torch.int32))      # the input, bit for bit
    assert torch.equal(got["out_triangles"], cuda(sphere["triangles"]))
    assert got["vertex_map"].tolist() == list(range(1418)) and got["triangle_map"].tolist() == list(range(2832))
    level = case("equal_to_level", 1)
    assert check_case(level, ("equal_to_level", 1), True, again=False)[0]["counts"][0].tolist() == [8689, 21864, 4622, 0, 5166, 0, 0, 0]
    assert check_case(level, ("equal_to_level", 1), False, again=False)[0]["counts"][0].tolist() == [13686, 21864, 4622, 0, 0, 169, 0, 0]
    tetra = case("duplicated_tetrahedron", 1)
    assert check_case(tetra, ("duplicated_tetrahedron", 1), True, again=False)[0]["counts"][0].tolist() == [4, 4, 0, 0, 8, 0, 0, 0]
    got, _ = check_case(ar.hand_made()[0], None, True, what="hand-made")
    assert got["counts"][0].tolist() == [4, 8, 9, 3, 2, 1, 0, 0] and got["vertex_map"].tolist() == [0, 1, 2, 3, 0, 1, -1, -1, -1, -1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the scans
def sliced_sphere(sizes):
    """Groups cut from the 17^3 sphere: the first ``V_g`` vertices and the first ``T_g`` triangles (tiled where the sphere is too
    small).  A triangle that refers to a vertex beyond ``V_g`` is dropped, and vertices are left unreferenced."""
    sphere = ir.part("sphere")[0]
    parts = []
    for V_g, T_g in sizes:
        repeat = -(-T_g // len(sphere["triangles"]))
        parts.append({"vertices": sphere["vertices"][:V_g], "triangles": np.tile(sphere["triangles"], (repeat, 1))[:T_g]})
    return ir.pack(parts)


@pytest.mark.parametrize("merge", [True, False], ids=["value", "compact_only"])
def test_groups_at_the_seams_of_the_block_scan(merge):
    sizes = [(255, 255), (256, 256), (257, 257), (513, 513), (255, 513), (513, 255), (256, 257), (1, 1), (257, 256)]
    mesh = sliced_sphere(sizes)
    assert np.diff(mesh["vertex_offsets"]).tolist() == [s[0] for s in sizes] and np.diff(mesh["triangle_offsets"]).tolist() == [s[1] for s in sizes]
    got, want = check_case(mesh, "seams", merge, width=1, with_normals=True)
    counts = want["counts"]
    print("seams:", counts[:, :6].tolist())
    assert (counts[:-2, 5] > 0).any() and (counts[:, 2] > 0).any() and (counts[:, 0] > 0).sum() >= 7      # unreferenced, dropped, and output


def test_one_group_above_256_x_256_elements_on_both_sides():
    n = 33
    field = np.random.default_rng(5).integers(-1, 2, (n, n, n)).astype(F) * F(0.5) + F(0.25)
    mesh = ir.pack([sr.extract_surface(field[None], [np.linspace(-1, 1, n).astype(F)] * 3, 0.25, normals=False)])
    got, want = check_case(mesh, None, True, what="33^3", again=False)
    assert (len(mesh["vertices"]), len(mesh["triangles"])) == (106440, 214426)
    assert got["counts"][0, :2].tolist() == [65970, 176106] and 65970 > 256 * 256 and 176106 > 256 * 256
    got, want = check_case(mesh, None, False, what="33^3 compact", again=False)
    assert got["counts"][0, 1].item() == 176106 and got["counts"][0, 0].item() > 65970


# ---------------------------------------------------------------------------------------------------------------------
# 3. attributes, optional outputs, capacities
@pytest.mark.parametrize("width", [1, 3, 192, 193])
def test_attribute_rows_are_the_representatives_bit_for_bit(width):
    mesh = case("equal_to_level", 3)
    for merge in (True, False):
        got, want = check_case(mesh, ("equal_to_level", 3), merge, width=width, with_normals=True, again=False, seed=width)
        assert got["out_attributes"].shape == (totals_of(want)[0], width)
        assert bool(torch.isnan(got["out_attributes"]).any()) and bool(torch.isnan(got["out_normals"]).any())
    # the rows are the REPRESENTATIVE's: vertex_map inverts them
    source = cuda(random_rows(len(mesh["vertices"]), width, 20 + width)).view(torch.int32)
    got, want = check_case(mesh, ("equal_to_level", 3), True, width=width, with_normals=True, again=False, seed=width)
    vo, out_vo = mesh["vertex_offsets"].tolist(), want["vertex_offsets"].tolist()
    for g in range(3):
        rep = cuda(ar.representatives(mesh["vertices"][vo[g]:vo[g + 1]]))
        own = torch.nonzero((rep == torch.arange(len(rep), device="cuda")) & (got["vertex_map"][vo[g]:vo[g + 1]] >= 0)).flatten()
        rows = got["vertex_map"][vo[g]:vo[g + 1]][own].long() + out_vo[g]
        assert torch.equal(got["out_attributes"].view(torch.int32)[rows], source[vo[g]:vo[g + 1]][own])
    # an attribute array that starts 4 bytes past a 16-byte boundary (whatever path the width alone would take): the same rows
    shifted = torch.empty(source.numel() + 1, dtype=torch.int32, device="cuda")[1:].view(source.shape)
    shifted.copy_(source)
    assert shifted.data_ptr() % 16 == 4
    normals = cuda(random_rows(len(mesh["vertices"]), 3, 10 + width))
    again = run_weld(device_mesh(mesh), totals_of(want), True, normals=normals, attributes=shifted.view(torch.float32))
    assert_weld_equal(again, want, ("shifted", width))


def test_optional_outputs_counting_calls_and_short_capacities():
    mesh = case("capped_noise", 3)
    V = len(mesh["vertices"])
    normals, attributes = random_rows(V, 3, 1), random_rows(V, 5, 2)
    dev = device_mesh(mesh)
    for merge in (True, False):
        want = wr.weld(mesh, merge, normals=normals, attributes=attributes)
        totals = totals_of(want)
        # normals and attributes omitted, each and both - as inputs, and as outputs only
        for n, a, on, oa in ((True, False, True, True), (False, True, True, True), (False, False, True, True), (True, True, False, True),
                             (True, True, True, False), (True, True, False, False)):
            got = run_weld(dev, totals, merge, normals=cuda(normals) if n else None, attributes=cuda(attributes) if a else None,
                           out_normals=on, out_attributes=oa)
            assert ("out_normals" in got) == (n and on) and ("out_attributes" in got) == (a and oa)
            assert_weld_equal(got, want, ("optional", merge, n, a, on, oa))
        # the maps omitted
        got = run_weld(dev, totals, merge, maps=False)
        assert "vertex_map" not in got and "triangle_map" not in got
        assert_weld_equal(got, want, ("no maps", merge))
        # a counting call writes nothing but counts and offsets (run_weld checks the workspace guard; there are no other outputs)
        got = run_weld(dev, totals, merge, normals=cuda(normals), attributes=cuda(attributes), emit=False, maps=False)
        assert set(got) == {"counts", "out_vertex_offsets", "out_triangle_offsets"}
        assert_weld_equal(got, want, ("counting", merge))
        # the maps alone
        got = run_weld(dev, totals, merge, emit=False, maps=True)
        assert_weld_equal(got, want, ("maps alone", merge))
        # capacities one short of the totals: the guards stay (run_weld), the rows in front are the reference's, the totals are true
        got = run_weld(dev, totals, merge, normals=cuda(normals), attributes=cuda(attributes), short=1)
        assert got["out_vertices"].size(0) == totals[0] - 1 and got["out_triangles"].size(0) == totals[1] - 1
        assert_weld_equal(got, want, ("short", merge))
        assert got["out_vertex_offsets"][-1].item() == totals[0] and got["out_triangle_offsets"][-1].item() == totals[1]


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate input
def test_five_groups_with_empty_ones_between_and_an_empty_input():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    parts = []
    for g, kind in enumerate(["torus", "all_outside", "noise", "all_inside", "sphere"]):
        field, level = make_field(kind, shape, axes, seed=50 + g)
        parts.append(sr.extract_surface(field[None], axes, level))
    mesh = ir.pack(parts)
    to = mesh["triangle_offsets"].tolist()
    assert to[1] == to[2] and to[3] == to[4] and to[0] < to[1] < to[3] < to[5]
    for merge in (True, False):
        got, want = check_case(mesh, None, merge, width=2, with_normals=True, what="five groups")
        assert not got["counts"][1].any() and not got["counts"][3].any() and int(got["counts"][0, 0]) > 0 and int(got["counts"][4, 0]) > 0
    # an entirely empty input
    empty = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32), "vertex_offsets": np.zeros(3, np.int32),
             "triangle_offsets": np.zeros(3, np.int32)}
    got, _ = check_case(empty, None, True, what="empty")
    assert not got["counts"].any() and not got["out_vertex_offsets"].any() and not got["out_triangle_offsets"].any()
    # vertices without triangles: every one is an unreferenced representative (or merged into one)
    lone = dict(empty, vertices=np.array([[1, 1, 1], [1, 1, 1], [2, 2, 2], [3, 3, 3], [2, 2, 2]], F), vertex_offsets=np.array([0, 2, 5], np.int32))
    got, _ = check_case(lone, None, True, what="lone")
    assert got["counts"].tolist() == [[0, 0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 1, 2, 0, 0]] and got["vertex_map"].tolist() == [-1] * 5
    got, _ = check_case(lone, None, False, what="lone compact")
    assert got["counts"].tolist() == [[0, 0, 0, 0, 0, 2, 0, 0], [0, 0, 0, 0, 0, 3, 0, 0]]


def test_hostile_meshes_and_offsets_cost_correctness_of_their_group_at_most():
    """The hand-made mesh between two clean ones, randomly broken meshes, and offsets that decrease, leave the arrays or arrive late:
    guards intact (``run_weld``), and every group - the reference clamps as the header says - equal to the reference."""
    hand, _ = ar.hand_made()
    sphere, torus = ir.part("sphere")[0], ir.part("torus")[0]
    mesh = ir.pack([sphere, hand, torus])
    for merge in (True, False):
        got, want = check_case(mesh, None, merge, width=2, with_normals=True, what="hand-made between")
        assert got["counts"][1].tolist() == ([4, 8, 9, 3, 2, 1, 0, 0] if merge else [6, 8, 9, 3, 0, 1, 0, 0])
        # the neighbours' rows are those of the clean meshes alone
        vo, to = want["vertex_offsets"].tolist(), want["triangle_offsets"].tolist()
        for g, clean in ((0, sphere), (2, torus)):
            assert torch.equal(got["out_vertices"][vo[g]:vo[g + 1]].view(torch.int32), cuda(clean["vertices"]).view(torch.int32))
            assert torch.equal(got["out_triangles"][to[g]:to[g + 1]], cuda(clean["triangles"]))
    base = case("sphere", 3)
    bad = hostile(base)
    V, T = len(base["vertices"]), len(base["triangles"])
    cases = [("values", bad)]
    for name, vo, to in (("decreasing", [0, base["vertex_offsets"][2], base["vertex_offsets"][1], V], [0, base["triangle_offsets"][2], base["triangle_offsets"][1], T]),
                         ("leaving", [-5, base["vertex_offsets"][1], V + 1000, 2 ** 31 - 1], [-2 ** 31, base["triangle_offsets"][1], T + 7, T + 9]),
                         ("late", [7, base["vertex_offsets"][1], base["vertex_offsets"][2], V - 3], [11, base["triangle_offsets"][1], base["triangle_offsets"][2], T - 5])):
        changed = dict(bad)
        changed["vertex_offsets"], changed["triangle_offsets"] = np.array(vo, dtype=np.int32), np.array(to, dtype=np.int32)
        cases.append((name, changed))
    for name, changed in cases:
        for merge in (True, False):
            got, want = check_case(changed, None, merge, width=2, with_normals=True, what=(name, merge), again=False)
            assert int(want["counts"][:, 2].sum()) > 0 and int(want["counts"][:, 1].sum()) > 0 and int(want["counts"][:, 3].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. a recorded call
@pytest.mark.parametrize("merge", [True, False], ids=["value", "compact_only"])
def test_recorded_call_holds_kernels_only_and_replays_on_a_smaller_mesh_and_back(merge):
    large, small = case("capped_noise", 3), case("sphere", 3)
    wants = [wr.weld(large, merge), wr.weld(small, merge)]
    devs = [device_mesh(large), device_mesh(small)]
    assert devs[1]["T"] < devs[0]["T"] and devs[1]["V"] < devs[0]["V"]
    # one set of buffers that holds either mesh: the totals the call is told are the capacities, the offsets say what is there
    V, T, G = devs[0]["V"], devs[0]["T"], 3
    held = {"vertices": torch.zeros((V, 3), device="cuda"), "triangles": torch.zeros((T, 3), dtype=torch.int32, device="cuda"),
            "vertex_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda"), "triangle_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda")}

    def load(which):
        dev = devs[which]
        held["vertices"][:dev["V"]].copy_(dev["vertices"][:dev["V"]])
        held["triangles"][:dev["T"]].copy_(dev["triangles"][:dev["T"]])
        held["vertex_offsets"].copy_(dev["vertex_offsets"])
        held["triangle_offsets"].copy_(dev["triangle_offsets"])

    load(0)
    rows = {"counts": G * 8, "out_vertex_offsets": G + 1, "out_triangle_offsets": G + 1, "out_vertices": V * 3, "out_triangles": T * 3,
            "vertex_map": V, "triangle_map": T}
    out = {key: poisoned((n + GUARD,), torch.float32 if key == "out_vertices" else torch.int32) for key, n in rows.items()}
    s = surface.weld_struct(held["vertices"], held["triangles"], held["vertex_offsets"], held["triangle_offsets"], V, T, merge=merge, **out)
    s.max_vertices, s.max_triangles = V, T
    lib = _lib.load()
    size = C.c_size_t()
    _lib.check(lib.pr_mesh_weld_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_weld_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")
    call = lambda: _lib.check(lib.pr_mesh_weld(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream), "pr_mesh_weld")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    census = frame_graph.node_census(graph)
    graph.instantiate()
    print("recorded weld:", census)
    assert census == {"nodes": KERNELS[merge], "kernels": KERNELS[merge], "memsets": 0, "memcpys": 0}
    for which in (0, 1, 0):
        want = wants[which]
        load(which)
        for t in out.values():
            t.view(torch.int32).fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        v, t = totals_of(want)
        got = {"counts": out["counts"][:G * 8].reshape(G, 8), "out_vertex_offsets": out["out_vertex_offsets"][:G + 1],
               "out_triangle_offsets": out["out_triangle_offsets"][:G + 1], "out_vertices": out["out_vertices"][:v * 3].reshape(v, 3),
               "out_triangles": out["out_triangles"][:t * 3].reshape(t, 3), "vertex_map": out["vertex_map"][:V], "triangle_map": out["triangle_map"][:T]}
        assert_weld_equal(got, want, ("replay", which))
        # nothing behind the true totals, nor behind the arrays, was written
        assert bool(is_poison(out["out_vertices"][v * 3:]).all()) and bool(is_poison(out["out_triangles"][t * 3:]).all())
        for key, n in rows.items():
            assert bool(is_poison(out[key][n:]).all()), key
        assert bool(is_poison(workspace[size.value // 4:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the consumers agree
def test_contains_closest_cast_and_audit_answer_identically_on_the_welded_mesh():
    mesh, axes = level_lattice_capped()
    whole = to_meshes(mesh)[0]
    welded, vertex_map, triangle_map = whole.welded(maps=True)
    assert 0 < welded.vertices.size(0) < whole.vertices.size(0) and 0 < welded.triangles.size(0) < whole.triangles.size(0)
    grid = surface.bounding_grid([whole], 16)
    points, _ = ir.point_batch(mesh, axes, 60, [ir.bounding_grid(mesh, (16, 16, 16)), ir.bounding_grid(mesh, (5, 7, 9))])
    points = cuda(points[0])
    points = points[torch.isfinite(points).all(dim=1)]
    assert points.size(0) >= 500
    before, after = surface.RayGrid.build([whole], *grid), surface.RayGrid.build([welded], *grid)
    for axis in (0, 1, 2):
        assert torch.equal(before.contains(points, axis=axis), after.contains(points, axis=axis))
    assert bool(before.contains(points).any()) and not bool(before.contains(points).all())
    tmap = lambda index: torch.where(index >= 0, triangle_map[index.clamp(min=0).long()], index)
    a, b = before.closest(points, max_distance=0.5), after.closest(points, max_distance=0.5)
    assert torch.equal(a.distance.view(torch.int32), b.distance.view(torch.int32)) and torch.equal(tmap(a.triangle[0]), b.triangle[0])
    assert bool((a.triangle >= 0).any()) and bool((b.triangle[0][a.triangle[0] >= 0] >= 0).all())
    directions = points.roll(1, dims=0) - points
    a, b = before.cast(points, directions), after.cast(points, directions)
    assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)) and torch.equal(tmap(a.triangle[0]), b.triangle[0])
    assert bool((a.triangle >= 0).any())
    # the audits: the counts but for `dropped`, the measures within the sum of the two stated bounds (the tree shifts)
    one, two = whole.audit(), welded.audit()
    want = one.counts.clone()
    assert int(want[1]) > 0
    want[1] = 0
    assert torch.equal(two.counts, want) and one.report()["balanced"]
    reference_in, reference_out = ar.audit(mesh), ar.audit(ir.pack([{"vertices": welded.vertices.cpu().numpy(), "triangles": welded.triangles.cpu().numpy()}]))
    bound = ar.bounds(reference_in)[0] + ar.bounds(reference_out)[0]
    error = (one.measures - two.measures).abs().cpu().numpy()
    print("measures of the input and of the welded mesh:", one.measures.tolist(), two.measures.tolist(), "error", error, "bound", bound)
    assert (error <= bound).all()
    # vertex_map: every finite input vertex that a kept triangle uses has its values at its output row
    used = vertex_map >= 0
    assert torch.equal(welded.vertices[vertex_map[used].long()], whole.vertices[used])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the python layer
def test_weld_meshes_mesh_welded_and_mesh_compacted_agree():
    mesh = case("equal_to_level", 3)
    V = len(mesh["vertices"])
    normals, features = random_rows(V, 3, 5), random_rows(V, 6, 6)
    vo = mesh["vertex_offsets"].tolist()
    meshes = to_meshes(mesh)
    for g, m in enumerate(meshes):
        m.normals, m.features = cuda(normals[vo[g]:vo[g + 1]]), cuda(features[vo[g]:vo[g + 1]])
    for merge in (True, False):
        want = wr.weld(mesh, merge, normals=normals, attributes=features)
        out_vo, out_to = want["vertex_offsets"].tolist(), want["triangle_offsets"].tolist()
        welded, vertex_maps, triangle_maps = surface.weld_meshes(meshes, merge=merge, maps=True)
        plain = surface.weld_meshes(meshes, merge=merge)
        assert len(welded) == len(plain) == 3
        bits = lambda t: t.view(torch.int32)
        for g, m in enumerate(meshes):
            alone = m.welded() if merge else m.compacted()
            with_maps = m.welded(merge=merge, maps=True)
            for other in (welded[g], plain[g], alone, with_maps[0]):
                assert other.vertices.dtype == torch.float32 and other.triangles.dtype == torch.int32 and other.features.dtype == torch.float32
                assert torch.equal(bits(other.vertices), bits(cuda(want["vertices"][out_vo[g]:out_vo[g + 1]])))
                assert torch.equal(other.triangles, cuda(want["triangles"][out_to[g]:out_to[g + 1]]))
                assert torch.equal(bits(other.normals), bits(cuda(want["normals"][out_vo[g]:out_vo[g + 1]])))
                assert torch.equal(bits(other.features), bits(cuda(want["attributes"][out_vo[g]:out_vo[g + 1]])))
            to = mesh["triangle_offsets"].tolist()
            for maps in ((vertex_maps[g], triangle_maps[g]), with_maps[1:]):
                assert torch.equal(maps[0], cuda(want["vertex_map"][vo[g]:vo[g + 1]])) and torch.equal(maps[1], cuda(want["triangle_map"][to[g]:to[g + 1]]))
    # normals / features are carried iff every input has them (features: with one common width); other dtypes come back as fp32
    meshes[1].normals = None
    meshes[2].features = meshes[2].features[:, :4]
    out = surface.weld_meshes(meshes)
    assert all(m.normals is None and m.features is None for m in out)
    half = surface.Mesh(meshes[0].vertices, meshes[0].triangles, None, torch.ones((meshes[0].vertices.size(0), 2), dtype=torch.float16, device="cuda"))
    out = half.welded()
    assert out.features.dtype == torch.float32 and bool((out.features == 1).all()) and out.normals is None
    # empty meshes
    empty = surface.Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    out, vertex_map, triangle_map = empty.welded(maps=True)
    assert out.vertices.shape == (0, 3) and out.triangles.shape == (0, 3) and vertex_map.numel() == 0 and triangle_map.numel() == 0
    lone = surface.Mesh(torch.ones((3, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    out, vertex_map, triangle_map = lone.welded(maps=True)
    assert out.vertices.shape == (0, 3) and vertex_map.tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="one row per vertex"):
        surface.Mesh(meshes[0].vertices, meshes[0].triangles, None, torch.ones((3, 2), device="cuda")).welded()


def test_keep_shells_compact_has_exactly_the_larger_spheres_rows():
    mesh = ar.two_spheres((0.27, 0.36))                                 # the larger sphere is the one at +0.47
    whole = to_meshes(mesh)[0]
    whole.normals = cuda(random_rows(len(mesh["vertices"]), 3, 9))
    loose, tidy = whole.keep_shells(1), whole.keep_shells(1, compact=True)
    # without compact: today's result
    labels = whole.audit(labels=True).labels
    larger = int(torch.bincount(labels.long()).argmax())
    assert loose.vertices is whole.vertices and loose.normals is whole.normals and torch.equal(loose.triangles, whole.triangles[labels == larger])
    # with it: exactly the larger sphere's vertices, in order, and its triangles re-indexed
    side = whole.vertices[:, 0] > 0
    assert torch.equal(tidy.vertices, whole.vertices[side]) and torch.equal(tidy.normals.view(torch.int32), whole.normals[side].view(torch.int32))
    assert tidy.triangles.size(0) == loose.triangles.size(0) and 0 < tidy.vertices.size(0) < whole.vertices.size(0)
    assert torch.equal(tidy.vertices[tidy.triangles.long()], whole.vertices[loose.triangles.long()])
    assert int(tidy.triangles.min()) == 0 and int(tidy.triangles.max()) == tidy.vertices.size(0) - 1
    report = tidy.audit().report()
    assert report["shells"] == 1 and report["closed_manifold"] and report["vertices"] == tidy.vertices.size(0)
    expected = surface.weld_meshes([loose], merge=False)[0]
    assert torch.equal(expected.vertices, tidy.vertices) and torch.equal(expected.triangles, tidy.triangles)


def test_extract_surface_weld_is_weld_meshes_of_the_unwelded_meshes():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    field, level = make_field("equal_to_level", shape, axes, seed=3)
    sigma = cuda(field[None])
    for kw in ({}, {"simplify": 2, "keep_duplicates": True, "close_border": True}, {"normals": False}):
        plain = surface.extract_surface(sigma, [cuda(a) for a in axes], level, **kw)
        welded = surface.extract_surface(sigma, [cuda(a) for a in axes], level, weld=True, **kw)
        want = surface.weld_meshes(plain)
        for a, b in zip(welded, want):
            assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
            assert (a.normals is None) == (b.normals is None) == ("normals" in kw)
            assert a.normals is None or torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
        assert welded[0].vertices.size(0) < plain[0].vertices.size(0) or kw.get("simplify")


# ---------------------------------------------------------------------------------------------------------------------
# 8. the composer
def test_extract_mesh_weld_welds_before_the_feature_query():
    """``extract_mesh(close_border=True, simplify=2, keep_duplicates=True, features=True)`` of the small tennis ``player_1`` network at
    resolution 24, level = the median: with ``weld=True`` the mesh is ``weld_meshes`` of the unwelded one in geometry, its features are
    those of a ``query_object`` at its own vertices, and its audit says what the unwelded one's says."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, _ = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        kw = dict(level=level, close_border=True, simplify=2, keep_duplicates=True, features=True)
        plain = comp.extract_mesh(PLAYER_1, 24, style, deformation, **kw)
        welded = comp.extract_mesh(PLAYER_1, 24, style, deformation, weld=True, **kw)
        want = surface.weld_meshes([surface.Mesh(m.vertices, m.triangles, m.normals) for m in plain])
        G, most = len(welded), max(m.vertices.size(0) for m in welded)
        points = welded[0].vertices[:1].expand(G, most, 3).clone()
        for g, m in enumerate(welded):
            points[g, :m.vertices.size(0)] = m.vertices
        features = comp.query_object(PLAYER_1, points, style, deformation)["features"]
    assert len(plain) == len(welded) == 2 and plain[0].triangles.size(0) > 0
    for g, (a, b, p) in enumerate(zip(welded, want, plain)):
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
        assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
        assert a.features.shape == (a.vertices.size(0), p.features.size(1)) and torch.equal(a.features, features[g, :a.vertices.size(0)])
        one, two = p.audit(), a.audit()
        expected = one.counts.clone()
        expected[1] = 0
        assert torch.equal(two.counts, expected) and one.report()["balanced"] and two.report()["balanced"]
        assert int(two.counts[2]) == a.vertices.size(0)               # every vertex is referenced and stands for one value
        print(f"group {g}: V {p.vertices.size(0)} -> {a.vertices.size(0)}, T {p.triangles.size(0)} -> {a.triangles.size(0)}")

"""Quadric placement on the GPU (python -m pytest tests -m gpu): ``pr_mesh_place`` against its numpy restatement
(tests/place_reference.py) - ``out_vertices`` and ``counts`` AS BITS - through the C ABI, every array in a poisoned allocation of its
own with guard words (tests/poisoned.py) and a poisoned workspace: spheres, boxes, a rotated box and a torus simplified on lattice
grids and on the off-lattice grid, groups of different sizes with an empty one, sizes at the seams of the blocks, one cluster for
everything, a cluster that only unreferenced vertices reach, hostile values, indices, map entries and offsets, equal bits from call to
call and under a permutation of the triangles, a recorded call replayed on other vertices, and the Python layer
(``simplify_meshes(placement="quadric")``, ``Mesh.simplified``, ``place_vertices``, ``extract_surface``, ``extract_mesh``, ``contains``)."""
import ctypes as C

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, surface
from tests import place_reference as pl
from tests import simplify_reference as sp
from tests import surface_reference as sr
from tests.poisoned import POISON, Placed
from tests.test_raycast_gpu import hostile, to_meshes
from tests.test_simplify_gpu import OFF_LATTICE
from tests.test_surface_gpu import PLAYER_1, codes, tennis

pytestmark = pytest.mark.gpu

F = np.float32
I = np.int32
KERNELS = 4                        # the header's launch count with merged triangles; one less without
REG = 2.0 ** -10


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# cases (numpy only), computed once and never changed
_CASES = {}


def box17(n=17, **kw):
    return pl.box_field(n, **kw)[:2]


FIELDS = {"sphere9": lambda: sr.sphere_field(9), "sphere17": lambda: sr.sphere_field(17), "box17": box17, "box9": lambda: box17(9),
          "rotated17": lambda: box17(rz=0.4, rx=0.3), "torus17": lambda: sr.torus_field(17),
          "outside9": lambda: (np.full((9, 9, 9), -1, F), [np.linspace(-1, 1, 9).astype(F)] * 3)}


def lattice_case(fields, k=2, grid=None):
    """The fine meshes of ``fields`` (one group each, all on the lattice of the first), simplified on the lattice grid of ``k`` steps
    per cell - or on ``grid`` - and described as ``pr_mesh_place`` reads them, with ``scale = max(cell)`` and ``max_move = cell``."""
    key = (tuple(fields), k, None if grid is None else "off")
    if key not in _CASES:
        parts = [sr.extract_surface(FIELDS[f]()[0][None], FIELDS[f]()[1], 0.0) for f in fields]
        mesh = {"vertices": np.concatenate([p["vertices"] for p in parts]), "normals": np.concatenate([p["normals"] for p in parts]),
                "triangles": np.concatenate([p["triangles"] for p in parts]),
                "vertex_offsets": np.concatenate([[0], np.cumsum([len(p["vertices"]) for p in parts])]).astype(I),
                "triangle_offsets": np.concatenate([[0], np.cumsum([len(p["triangles"]) for p in parts])]).astype(I)}
        origin, cell, cells = sp.lattice_grid(FIELDS[fields[0]]()[1], k) if grid is None else grid
        _CASES[key] = described(mesh, sp.simplify_mesh(mesh, origin, cell, cells), max(cell), cell)
    return _CASES[key]


def described(mesh, simplified, scale, max_move):
    return {"vertices": mesh["vertices"], "triangles": mesh["triangles"], "vertex_offsets": mesh["vertex_offsets"],
            "triangle_offsets": mesh["triangle_offsets"], "vertex_map": simplified["vertex_map"], "merged_vertices": simplified["vertices"],
            "merged_vertex_offsets": simplified["vertex_offsets"], "merged_triangles": simplified["triangles"],
            "merged_triangle_offsets": simplified["triangle_offsets"], "scale": scale, "max_move": list(max_move), "regularisation": REG}


def random_case(sizes, seed=0, clusters_near=True):
    """Groups of ``(V, T, VO, TO)`` rows of random vertices in the unit cube, random triangles, a random map and random merged
    triangles: nothing a mesher would make, every size the blocks can meet."""
    rng = np.random.default_rng(seed)
    v, t, vmap, m, u = [], [], [], [], []
    for V, T, VO, TO in sizes:
        v.append(rng.uniform(0, 1, (V, 3)).astype(F))
        t.append(rng.integers(0, max(V, 1), (T, 3)).astype(I))
        vmap.append(rng.integers(0, max(VO, 1), V).astype(I))
        m.append(rng.uniform(0.25, 0.75, (VO, 3)).astype(F))
        u.append(rng.integers(0, max(VO, 1), (TO, 3)).astype(I))
    offsets = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(I)
    return {"vertices": np.concatenate(v), "triangles": np.concatenate(t), "vertex_offsets": offsets(v), "triangle_offsets": offsets(t),
            "vertex_map": np.concatenate(vmap), "merged_vertices": np.concatenate(m), "merged_vertex_offsets": offsets(m),
            "merged_triangles": np.concatenate(u), "merged_triangle_offsets": offsets(u), "scale": 0.5, "max_move": [0.5, 0.25, 0.5],
            "regularisation": REG}


def poison_rows(rows):
    return np.full(rows * 3, POISON, np.uint32).view(F).reshape(rows, 3)


def reference(case, merged_triangles=True):
    """``pl.place`` on an output that holds the poison pattern: what no clamped group owns stays poisoned."""
    return pl.place(case["vertices"], case["triangles"], case["vertex_offsets"], case["triangle_offsets"], case["vertex_map"],
                    case["merged_vertices"], case["merged_vertex_offsets"], scale=case["scale"], max_move=case["max_move"],
                    regularisation=case["regularisation"], merged_triangles=case["merged_triangles"] if merged_triangles else None,
                    merged_triangle_offsets=case["merged_triangle_offsets"] if merged_triangles else None,
                    out=poison_rows(len(case["merged_vertices"])))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
INPUTS = (("vertices", F), ("triangles", I), ("vertex_offsets", I), ("triangle_offsets", I), ("vertex_map", I), ("merged_vertices", F),
          ("merged_vertex_offsets", I), ("merged_triangles", I), ("merged_triangle_offsets", I))


class Call:
    """The arrays of a case in poisoned allocations, a description of them, a poisoned workspace: ``run`` makes the call,
    ``results`` reads the outputs back and checks every guard and that no input was written."""

    def __init__(self, case, merged_triangles=True):
        self.case = case
        self.inputs = {name: Placed(case[name], dtype=dtype) for name, dtype in INPUTS if merged_triangles or not name.startswith("merged_t")}
        G, VO = len(case["vertex_offsets"]) - 1, len(case["merged_vertices"])
        self.G, self.VO = G, VO
        self.out = Placed.poisoned(VO * 3)
        self.counts = Placed.poisoned(G * 4, dtype=I)
        s = _lib.MeshPlace()
        s.groups, s.total_vertices, s.total_triangles, s.flags = G, len(case["vertices"]), len(case["triangles"]), 0
        s.total_merged_vertices, s.total_merged_triangles = VO, len(case["merged_triangles"]) if merged_triangles else 0
        s.scale, s.regularisation = case["scale"], case["regularisation"]
        for a in range(3):
            s.max_move[a] = case["max_move"][a]
        for name, placed in self.inputs.items():
            setattr(s, name, placed.pointer)
        s.out_vertices, s.counts = self.out.pointer, self.counts.pointer
        self.s = s
        size = C.c_size_t()
        self.lib = _lib.load()
        _lib.check(self.lib.pr_mesh_place_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_place_workspace_size")
        self.size = size.value
        self.workspace = torch.full((self.size // 4 + 64,), POISON, dtype=torch.int32, device="cuda")       # (64 guard words)

    def run(self):
        _lib.check(self.lib.pr_mesh_place(C.byref(self.s), self.workspace.data_ptr(), self.size, torch.cuda.current_stream().cuda_stream),
                   "pr_mesh_place")

    def results(self, what):
        torch.cuda.synchronize()
        assert bool((self.workspace[self.size // 4:] == POISON).all()), (what, "workspace guard")
        for name, placed in self.inputs.items():
            placed.unchanged(f"{what}: {name}")
        return {"vertices": self.out.read(f"{what}: out_vertices").reshape(self.VO, 3), "counts": self.counts.read(f"{what}: counts").reshape(self.G, 4)}


def assert_equal_bits(got, want, what):
    for key in ("vertices", "counts"):
        a, b = got[key].view(np.uint32), np.ascontiguousarray(want[key]).view(np.uint32)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        wrong = np.argwhere(a != b)
        assert not len(wrong), (what, key, len(wrong), wrong[:4].tolist(), got[key][tuple(wrong[0])], want[key][tuple(wrong[0])])


def check_case(case, what, merged_triangles=True, again=False):
    want = reference(case, merged_triangles)
    call = Call(case, merged_triangles)
    call.run()
    got = call.results(what)
    assert_equal_bits(got, want, what)
    if again:                                                           # the same call into fresh buffers: equal bits
        second = Call(case, merged_triangles)
        second.run()
        assert_equal_bits(second.results((what, "again")), got, (what, "again"))
    return got, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes
SHAPES = [("sphere9", 2), ("sphere17", 2), ("box17", 2), ("box17", 4), ("rotated17", 2), ("torus17", 2)]


@pytest.mark.parametrize("field,k", SHAPES, ids=[f"{f}-{k}" for f, k in SHAPES])
def test_placement_equals_the_reference(field, k):
    case = lattice_case((field,), k)
    got, want = check_case(case, (field, k), again=True)
    counts = got["counts"][0].tolist()
    print(f"{field} k={k}: V {len(case['vertices'])} T {len(case['triangles'])} -> VO {len(case['merged_vertices'])} "
          f"TO {len(case['merged_triangles'])}, counts {counts}")
    assert counts[0] == len(case["merged_vertices"]) > 0 and counts[1] == counts[2] == 0      # every cluster moved, nothing was skipped
    assert (counts[3] == 0) or field == "rotated17"
    assert not np.array_equal(got["vertices"], case["merged_vertices"])
    without, _ = check_case(case, (field, k, "no merged triangles"), merged_triangles=False)
    assert np.array_equal(without["vertices"].view(np.uint32), got["vertices"].view(np.uint32)) and without["counts"][0].tolist() == counts[:3] + [0]


def test_the_off_lattice_grid():
    case = lattice_case(("sphere17",), grid=OFF_LATTICE)
    got, _ = check_case(case, "off lattice", again=True)
    assert got["counts"][0, 0] > 0 and got["counts"][0, :2].sum() == len(case["merged_vertices"])


def test_three_groups_of_different_sizes_with_an_empty_one():
    case = lattice_case(("sphere17", "outside9", "box9"))
    sizes = np.diff(case["merged_vertex_offsets"]).tolist()
    assert sizes[1] == 0 and sizes[0] > sizes[2] > 0 and np.diff(case["triangle_offsets"]).tolist()[1] == 0
    got, _ = check_case(case, "three groups", again=True)
    assert got["counts"][:, :2].sum(axis=1).tolist() == sizes and got["counts"][0, 0] == sizes[0] and not got["counts"][1].any()
    # every group alone gives its rows
    alone = lattice_case(("sphere17",))
    one, _ = check_case(alone, "alone")
    assert np.array_equal(one["vertices"].view(np.uint32), got["vertices"][:sizes[0]].view(np.uint32))


def test_sizes_at_the_seams_of_the_blocks_and_empty_input():
    sizes = [(1, 1, 1, 1), (255, 255, 255, 255), (257, 257, 257, 257), (0, 0, 0, 0), (257, 255, 1, 0), (1, 257, 255, 257), (255, 0, 257, 1),
             (0, 255, 0, 255), (256, 256, 256, 256), (513, 1100, 3, 255)]
    got, want = check_case(random_case(sizes), "seams", again=True)
    print("seams:", got["counts"].tolist())
    assert (want["counts"][:, 0] > 0).sum() >= 5 and (want["counts"][:, 1] > 0).sum() >= 5 and want["counts"][:, 3].sum() > 0
    assert want["counts"][:, 2].sum() > 0                               # (random triangles repeat an index now and then: no area, skipped)
    empty, _ = check_case(random_case([(0, 0, 0, 0)] * 3), "empty")
    assert not empty["counts"].any() and empty["vertices"].size == 0
    check_case(random_case(sizes), "seams, no merged triangles", merged_triangles=False)


def test_all_triangles_in_one_cluster_and_a_cluster_of_unreferenced_vertices():
    # one cluster for a whole mesh: every run of the wave-level merge is a full wave
    case = dict(lattice_case(("sphere17",)))
    V = len(case["vertices"])
    centre = case["vertices"].astype(np.float64).mean(axis=0).astype(F)[None]
    for name, vmap, merged in (("one cluster", np.zeros(V, I), centre), ("one of three", np.full(V, 1, I), np.concatenate([centre + F(1), centre, centre - F(1)]))):
        one = dict(case, vertex_map=vmap, merged_vertices=merged, merged_vertex_offsets=np.array([0, len(merged)], I),
                   merged_triangles=np.zeros((0, 3), I), merged_triangle_offsets=np.zeros(2, I), scale=1.0, max_move=[1.0] * 3)
        got, want = check_case(one, name, again=True)
        print(name, got["counts"].tolist(), got["vertices"].tolist())
        assert got["counts"][0, :2].sum() == len(merged) and got["counts"][0, 2] == 0
        assert np.array_equal(np.delete(got["vertices"], len(merged) // 2, axis=0).view(np.uint32), np.delete(merged, len(merged) // 2, axis=0).view(np.uint32))
    # vertices that no triangle refers to, alone in their cells: those clusters keep their means bit for bit
    base = sr.extract_surface(sr.sphere_field(17)[0][None], sr.sphere_field(17)[1], 0.0)
    lone = np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.04], [-0.9, -0.9, -0.9]], F)
    mesh = dict(base, vertices=np.concatenate([base["vertices"], lone]), normals=np.concatenate([base["normals"], np.zeros((3, 3), F)]),
                vertex_offsets=np.array([0, len(base["vertices"]) + 3], I))
    origin, cell, cells = sp.lattice_grid(sr.sphere_field(17)[1], 2)
    simp = sp.simplify_mesh(mesh, origin, cell, cells)
    got, _ = check_case(described(mesh, simp, max(cell), cell), "unreferenced")
    added = np.unique(simp["vertex_map"][-3:])
    assert got["counts"][0].tolist()[:3] == [len(simp["vertices"]) - 2, 2, 0] and len(added) == 2
    assert np.array_equal(got["vertices"][added].view(np.uint32), simp["vertices"][added].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. hostile input
def test_hostile_values_indices_map_entries_and_offsets_cost_correctness_of_their_group_at_most():
    """NaN and infinite vertices, triangle indices out of range, map entries out of range, merged vertices that are not finite,
    merged triangles out of range, and offsets that decrease, leave the arrays or leave rows unowned: every guard intact, no input
    written (``Call.results``), every row equal to the reference - which clamps as the header says and leaves unowned rows alone."""
    base = lattice_case(("sphere17", "box17", "torus17"))
    rng = np.random.default_rng(2)
    fine = hostile({k: base[k] for k in ("vertices", "triangles", "vertex_offsets", "triangle_offsets")})
    bad = dict(base, **fine)
    bad["vertex_offsets"], bad["triangle_offsets"] = base["vertex_offsets"], base["triangle_offsets"]
    got, want = check_case(bad, "values and indices", again=True)
    assert (want["counts"][:, 2] > 0).all() and (want["counts"][:, 0] > 0).all()
    # map entries: -1, VO_g, 2^31 - 1, -2^31
    vmap = base["vertex_map"].copy()
    pick = rng.uniform(0, 1, len(vmap))
    vo, mo = base["vertex_offsets"], base["merged_vertex_offsets"]
    for g in range(3):
        rows = np.arange(vo[g], vo[g + 1])
        vmap[rows[pick[rows] < 0.02]] = -1
        vmap[rows[(pick[rows] >= 0.02) & (pick[rows] < 0.04)]] = mo[g + 1] - mo[g]
        vmap[rows[(pick[rows] >= 0.04) & (pick[rows] < 0.05)]] = 2 ** 31 - 1
        vmap[rows[(pick[rows] >= 0.05) & (pick[rows] < 0.06)]] = -2 ** 31
    got, want = check_case(dict(bad, vertex_map=vmap), "map entries")
    assert (want["counts"][:, 0] > 0).all()
    # the merged mesh: vertices that are not finite, triangles out of range
    merged, u = base["merged_vertices"].copy(), base["merged_triangles"].copy()
    pick = rng.uniform(0, 1, merged.shape)
    merged[pick < 0.01], merged[(pick >= 0.01) & (pick < 0.02)] = np.nan, np.inf
    pick = rng.uniform(0, 1, len(u))
    u[pick < 0.03, 1], u[(pick >= 0.03) & (pick < 0.06), 2], u[(pick >= 0.06) & (pick < 0.07), 0] = -1, 2 ** 31 - 1, len(merged)
    got, want = check_case(dict(bad, vertex_map=vmap, merged_vertices=merged, merged_triangles=u), "merged mesh")
    assert (want["counts"][:, 1] > 0).all() and (want["counts"][:, 2] > 0).all()
    # offsets
    V, T, VO, TO = len(base["vertices"]), len(base["triangles"]), len(merged), len(u)
    to, uo = base["triangle_offsets"], base["merged_triangle_offsets"]
    for name, v_off, t_off, m_off, u_off in (
            ("decreasing", [0, vo[2], vo[1], V], [0, to[2], to[1], T], [0, mo[2], mo[1], VO], [0, uo[2], uo[1], TO]),
            ("leaving", [-5, vo[1], V + 1000, 2 ** 31 - 1], [-2 ** 31, to[1], T + 7, T + 9], [-1, mo[1], VO + 1, 2 ** 31 - 1], [-7, uo[1], TO + 3, TO + 4]),
            ("unowned rows", [7, vo[1], vo[2], V - 3], [11, to[1], to[2], T - 5], [5, mo[1], mo[2], VO - 4], [3, uo[1], uo[2], TO - 2])):
        changed = dict(bad, vertex_map=vmap, merged_vertices=merged, merged_triangles=u, vertex_offsets=np.array(v_off, I),
                       triangle_offsets=np.array(t_off, I), merged_vertex_offsets=np.array(m_off, I), merged_triangle_offsets=np.array(u_off, I))
        got, want = check_case(changed, name)
        assert want["counts"][:, :2].sum() > 0
        if name == "unowned rows":                                      # not touched: the poison is still there
            assert (got["vertices"][:5].view(np.uint32) == POISON).all() and (got["vertices"][-4:].view(np.uint32) == POISON).all()
            assert not (got["vertices"][5:-4].view(np.uint32) == POISON).any()
    # a clean group between hostile ones is the clean mesh's alone
    clean = dict(bad)
    clean["vertices"], clean["triangles"] = bad["vertices"].copy(), bad["triangles"].copy()
    clean["vertices"][vo[1]:vo[2]], clean["triangles"][to[1]:to[2]] = base["vertices"][vo[1]:vo[2]], base["triangles"][to[1]:to[2]]
    got, _ = check_case(clean, "clean between")
    alone, _ = check_case(lattice_case(("box17",)), "box alone")
    assert np.array_equal(got["vertices"][mo[1]:mo[2]].view(np.uint32), alone["vertices"].view(np.uint32)) and got["counts"][1].tolist() == alone["counts"][0].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 3. repeatability
def test_the_order_of_the_triangles_does_not_show():
    case = lattice_case(("sphere17", "box17", "torus17"))
    first, _ = check_case(case, "in order", again=True)
    order = []
    rng = np.random.default_rng(9)
    for g in range(3):                                                  # a permutation inside every group
        order.append(case["triangle_offsets"][g] + rng.permutation(case["triangle_offsets"][g + 1] - case["triangle_offsets"][g]))
    shuffled = dict(case, triangles=case["triangles"][np.concatenate(order)])
    second, _ = check_case(shuffled, "permuted")
    assert_equal_bits(second, first, "permuted against in order")


def test_a_recorded_call_holds_kernels_only_and_replays_on_other_vertices():
    case = lattice_case(("sphere17", "box17", "torus17"))
    moved = dict(case, vertices=(case["vertices"] * F(0.97) + F(0.004)).astype(F), merged_vertices=(case["merged_vertices"] * F(0.97) + F(0.004)).astype(F))
    wants = [reference(case), reference(moved)]
    assert not np.array_equal(wants[0]["vertices"], wants[1]["vertices"])
    for merged_triangles in (True, False):
        call = Call(case, merged_triangles)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call.run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            call.run()
        census = frame_graph.node_census(graph)
        graph.instantiate()
        kernels = KERNELS if merged_triangles else KERNELS - 1
        print("recorded placement:", census)
        assert census == {"nodes": kernels, "kernels": kernels, "memsets": 0, "memcpys": 0}
        for which in (1, 0, 1):
            source = (case, moved)[which]
            for name in ("vertices", "merged_vertices"):
                call.inputs[name].view.copy_(torch.from_numpy(source[name].reshape(-1)))
                call.inputs[name].sent = source[name].reshape(-1).copy()
            call.out.view.view(torch.int32).fill_(POISON)
            call.counts.view.fill_(POISON)
            graph.replay()
            want = wants[which] if merged_triangles else dict(wants[which], counts=wants[which]["counts"] * np.array([1, 1, 1, 0], I))
            assert_equal_bits(call.results(("replay", which)), want, ("replay", which, merged_triangles))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the python layer
def packed_of(meshes):
    sizes = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(I)
    return {"vertices": torch.cat([m.vertices for m in meshes]).cpu().numpy(), "normals": torch.cat([m.normals for m in meshes]).cpu().numpy(),
            "triangles": torch.cat([m.triangles for m in meshes]).cpu().numpy(), "vertex_offsets": sizes([m.vertices for m in meshes]),
            "triangle_offsets": sizes([m.triangles for m in meshes])}


def assert_meshes_are(meshes, simplified, placed, what):
    vo, to = simplified["vertex_offsets"], simplified["triangle_offsets"]
    assert len(meshes) == len(vo) - 1
    for g, m in enumerate(meshes):
        assert torch.equal(m.vertices.view(torch.int32), cuda(placed["vertices"][vo[g]:vo[g + 1]]).view(torch.int32)), (what, g, "vertices")
        assert torch.equal(m.triangles, cuda(simplified["triangles"][to[g]:to[g + 1]])), (what, g, "triangles")
        assert torch.equal(m.normals.view(torch.int32), cuda(simplified["normals"][vo[g]:vo[g + 1]]).view(torch.int32)), (what, g, "normals")


def test_simplify_meshes_mesh_simplified_and_place_vertices():
    fields = ("sphere17", "outside9", "box9")
    case = lattice_case(fields)
    axes = FIELDS["sphere17"]()[1]
    origin, cell, cells = sp.lattice_grid(axes, 2)
    fine = {k: case[k] for k in ("vertices", "triangles", "vertex_offsets", "triangle_offsets")}
    normals = np.concatenate([sr.extract_surface(FIELDS[f]()[0][None], FIELDS[f]()[1], 0.0)["normals"] for f in fields])
    meshes = to_meshes(fine)
    vo = fine["vertex_offsets"]
    for g, m in enumerate(meshes):
        m.normals = cuda(normals[vo[g]:vo[g + 1]])
    simplified = sp.simplify_mesh(dict(fine, normals=normals), origin, cell, cells)
    placed = pl.place_simplified(fine, simplified, cell)
    for keep in (False, True):
        kept = sp.simplify_mesh(dict(fine, normals=normals), origin, cell, cells, keep_duplicates=keep)
        want = pl.place_simplified(fine, kept, cell)
        got = surface.simplify_meshes(meshes, origin, cell, cells, placement="quadric", keep_duplicates=keep)
        assert_meshes_are(got, kept, want, ("simplify_meshes", keep))
        for g in (0, 2):                                                # a mesh alone is its group
            alone = meshes[g].simplified(origin, cell, cells, placement="quadric", keep_duplicates=keep)
            assert torch.equal(alone.vertices.view(torch.int32), got[g].vertices.view(torch.int32)) and torch.equal(alone.triangles, got[g].triangles)
    # "mean" is the call without the argument, bit for bit
    plain = surface.simplify_meshes(meshes, origin, cell, cells)
    mean = surface.simplify_meshes(meshes, origin, cell, cells, placement="mean")
    quadric = surface.simplify_meshes(meshes, origin, cell, cells, placement="quadric")
    for a, b, c in zip(plain, mean, quadric):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.triangles, b.triangles) and torch.equal(a.normals, b.normals)
        assert torch.equal(a.triangles, c.triangles) and torch.equal(a.normals, c.normals)
        assert a.vertices.size(0) == 0 or not torch.equal(a.vertices, c.vertices)
    # place_vertices: the call on its own, features and normals carried
    vmaps = [cuda(simplified["vertex_map"][vo[g]:vo[g + 1]]) for g in range(3)]
    for m in plain:
        m.features = torch.randn(m.vertices.size(0), 3, device="cuda")
    out, counts = surface.place_vertices(meshes, plain, vmaps, scale=max(cell), max_move=cell)
    assert counts.dtype == torch.int32 and counts.is_cuda and torch.equal(counts, cuda(placed["counts"]))
    assert_meshes_are(out, simplified, placed, "place_vertices")
    for a, b in zip(out, plain):
        assert a.triangles is b.triangles and a.normals is b.normals and a.features is b.features
    one, count = surface.place_vertices(meshes[:1], plain[:1], vmaps[:1], scale=max(cell), max_move=cell)
    assert torch.equal(one[0].vertices.view(torch.int32), out[0].vertices.view(torch.int32)) and torch.equal(count, counts[:1])
    still, count = surface.place_vertices(meshes, plain, vmaps, scale=max(cell), max_move=0.0)
    assert all(torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) for a, b in zip(still, plain))
    with pytest.raises(ValueError, match="placement must be one of"):
        surface.simplify_meshes(meshes, origin, cell, cells, placement="qem")


def test_extract_surface_and_extract_mesh_place_on_the_calls_own_mesh():
    """The small tennis ``player_1`` network at 12^3, level = the median: ``extract_surface(simplify=2, placement="quadric")`` and
    ``extract_mesh`` of the same are the reference's simplification and placement of the call's own unsimplified mesh; the features are
    queried at the placed vertices (clamped to the lattice hull)."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 12, style, deformation)
        level = float(sigma.median())
        plain = comp.extract_mesh(PLAYER_1, 12, style, deformation, level=level)
        mean = comp.extract_mesh(PLAYER_1, 12, style, deformation, level=level, simplify=2, features=True)
        same = comp.extract_mesh(PLAYER_1, 12, style, deformation, level=level, simplify=2, features=True, placement="mean")
        got = comp.extract_mesh(PLAYER_1, 12, style, deformation, level=level, simplify=2, features=True, placement="quadric")
    axes = [centres[:, 0, 0, 0], centres[0, :, 0, 1], centres[0, 0, :, 2]]
    host_axes = [a.cpu().numpy() for a in axes]
    packed = packed_of(plain)
    origin, cell, cells = sp.lattice_grid(host_axes, 2)
    simplified = sp.simplify_mesh(packed, origin, cell, cells)
    placed = pl.place_simplified(packed, simplified, cell)
    print(f"tennis 12^3: V {packed['vertex_offsets'].tolist()} -> {simplified['vertex_offsets'].tolist()}, counts {placed['counts'].tolist()}")
    assert placed["counts"][:, 0].min() > 0
    assert_meshes_are(got, simplified, placed, "extract_mesh")
    assert_meshes_are(surface.extract_surface(sigma, axes, level, simplify=2, placement="quadric"), simplified, placed, "extract_surface")
    for a, b in zip(mean, same):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.triangles, b.triangles) and torch.equal(a.features, b.features)
    lo, hi = torch.stack([a[0] for a in axes]), torch.stack([a[-1] for a in axes])
    with torch.no_grad():
        for g, m in enumerate(got):
            want = comp.query_object(PLAYER_1, torch.maximum(torch.minimum(m.vertices, hi), lo), style[g], deformation[g])["features"]
            assert torch.equal(m.features, want) and not torch.equal(m.features, mean[g].features)
    # through the weld and the smoothing: the placement comes first
    welded = surface.extract_surface(sigma, axes, level, simplify=2, placement="quadric", weld=True)
    want = surface.weld_meshes(surface.extract_surface(sigma, axes, level, simplify=2, placement="quadric"))
    assert all(torch.equal(a.vertices, b.vertices) and torch.equal(a.triangles, b.triangles) for a, b in zip(welded, want))
    with pytest.raises(ValueError, match="placement must be one of"):
        surface.extract_surface(sigma, axes, level, simplify=2, placement="lindstrom")


def test_contains_on_a_capped_quadric_mesh_answers_the_lattices_own_inside_away_from_the_surface():
    """``keep_duplicates=True`` and ``close_border=True`` with the quadric placement: the triangle lists are the mean rule's, so the
    mesh is still a cycle and ``contains`` decides.  At the lattice points further than a cluster cell (0.125) from the sphere - ten
    times the largest distance of a placed vertex from the true surface at this size (0.0025) - it answers the
    lattice's own inside, on all three axes."""
    n = 33
    field, axes = sr.sphere_field(n)
    sigma, device_axes = cuda(field[None]), [cuda(a) for a in axes]
    kw = dict(close_border=True, simplify=2, keep_duplicates=True)
    mean = surface.extract_surface(sigma, device_axes, 0.0, **kw)[0]
    quadric = surface.extract_surface(sigma, device_axes, 0.0, placement="quadric", **kw)[0]
    assert torch.equal(mean.triangles, quadric.triangles) and not torch.equal(mean.vertices, quadric.vertices)
    a, b = mean.audit(), quadric.audit()
    assert torch.equal(a.counts, b.counts) and a.report()["balanced"] and b.report()["balanced"]
    volumes = [abs(x.report()["signed_volume"]) / (4 / 3 * np.pi * 0.63 ** 3) - 1 for x in (a, b)]
    print(f"sphere 33^3, 2 steps per cell: V {quadric.vertices.size(0)}, T {quadric.triangles.size(0)}, volume error "
          f"{100 * volumes[0]:+.2f} % -> {100 * volumes[1]:+.2f} %")
    assert abs(volumes[1]) < abs(volumes[0])
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    points = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    radius = np.linalg.norm(points.astype(np.float64), axis=1)
    away = np.abs(radius - 0.63) > 0.125
    assert away.sum() > points.shape[0] // 2 and 0 < (radius[away] < 0.63).sum()
    grid = surface.RayGrid.build([quadric], *surface.bounding_grid([quadric], 16))
    for axis in range(3):
        inside = grid.contains(cuda(points[away].astype(F)), axis=axis)[0]
        assert torch.equal(inside, cuda(field.reshape(-1)[away] > 0)), axis

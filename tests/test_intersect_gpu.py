"""Mesh intersection on the GPU (python -m pytest tests -m gpu): ``pr_mesh_intersect`` against the exhaustive numpy rule
(tests/intersect_reference.py) bit for bit - ``count``, ``first``, ``pair_offsets``, the sorted ``pairs`` and ``segments`` as bits - on
the meshes of tests/surface_reference.py and the five grids of tests/test_raycast_gpu.py, in one and three groups, posed by a
transform, with the lattice-aligned shift; poisoned outputs with guard rows, every optional combination of outputs, short capacities,
hostile and stale input, self mode, repeated and recorded calls; the Python layer and ``ObjectComposer.extract_mesh`` on the small
tennis networks.  The reference does not depend on the grid, so one table per (meshes, transform) serves all grids."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, frame_graph, surface
from tests import intersect_reference as ir
from tests import simplify_reference as sp
from tests import surface_reference as sr
from tests.test_raycast_gpu import GRIDS, OFF_LATTICE, device_mesh, hostile, lists_of, make_grid, pack, run_build, to_meshes
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, poisoned, tennis

pytestmark = pytest.mark.gpu

F = np.float32
OUTPUTS = ("first", "pair_offsets", "pairs", "segments")
SHIFT = (0.3, 0.1, 0.05)
ALIGNED = (0.5, 0.5, 0.0)                                   # four lattice steps of the 17^3 lattice on two axes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes, transforms, reference tables (numpy only: nothing here needs a GPU)
_PARTS, _CASES, _WANT = {}, {}, {}
AXES = {n: [np.linspace(-1, 1, n).astype(F)] * 3 for n in (9, 17)}
EMPTY = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32)}


def part(kind, n=9):
    if (kind, n) not in _PARTS:
        field, axes = (sr.sphere_field if kind == "sphere" else sr.torus_field)(n)
        _PARTS[(kind, n)] = ir.packed(sr.extract_surface(field[None], axes, 0.0, normals=False))
    return _PARTS[(kind, n)]


def pose(degrees=25.0, shift=(0.2, -0.1, 0.15)):
    """A rotation about (1, 2, 3) plus a shift, as a (3, 4) fp32 matrix."""
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    a = math.radians(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K
    return np.concatenate([R, np.asarray(shift, dtype=np.float64)[:, None]], axis=1).astype(F)


def case(name):
    """(target, query, transform (G, 3, 4) or None) - packed dicts."""
    if name not in _CASES:
        sphere, torus = part("sphere"), part("torus")
        if name == "sphere_shifted":
            c = (sphere, ir.shifted(sphere, SHIFT), None)
        elif name == "sphere_torus":
            c = (sphere, torus, None)
        elif name == "three_groups":                        # different sizes, one target empty
            c = (pack([sphere, EMPTY, torus]), pack([ir.shifted(sphere, SHIFT), torus, sphere]), None)
        elif name == "posed":
            c = (sphere, torus, pose()[None])
        elif name == "posed_groups":
            c = (pack([sphere, EMPTY, torus]), pack([sphere, torus, sphere]),
                 np.stack([pose(), pose(70.0, (0, 0, 0)), pose(-40.0, (0.1, 0.3, -0.2))]))
        elif name == "aligned17":
            big = part("sphere", 17)
            c = (big, ir.shifted(big, ALIGNED), None)
        else:
            raise KeyError(name)
        _CASES[name] = c
    return _CASES[name]


def reference(name):
    if name not in _WANT:
        target, query, transform = case(name)
        _WANT[name] = ir.intersect(target, query, transform)
    return _WANT[name]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def call(dev, grid, built, qdev, transform, self_, out, pairs=None, segments=None, capacity=None):
    cell_offsets, references, R = built
    q = {} if self_ else dict(q_vertices=qdev["vertices"], q_triangles=qdev["triangles"], q_vertex_offsets=qdev["vertex_offsets"],
                              q_triangle_offsets=qdev["triangle_offsets"], q_total_vertices=qdev["V"], q_total_triangles=qdev["T"])
    s = surface.intersect_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                                 cell_offsets, references=references[:R] if R else None, transform=transform, count=out["count"],
                                 first=out.get("first"), pair_offsets=out.get("pair_offsets"), pairs=pairs, segments=segments,
                                 self_=self_, **q)
    if capacity is not None:
        s.max_pairs = capacity
    size = C.c_size_t()
    _lib.check(_lib.load().pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_intersect_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")          # (64 guard words)
    return s, workspace, size.value


def launch(s, workspace, size):
    _lib.check(_lib.load().pr_mesh_intersect(C.byref(s), workspace.data_ptr(), size, torch.cuda.current_stream().cuda_stream), "pr_mesh_intersect")


def run_intersect(target, grid, query=None, transform=None, self_=False, outputs=OUTPUTS, capacity=None, built=None):
    """A counting call, the read-back of P and (with "pairs") an emitting call with ``capacity`` (default: P) rows, all on poisoned
    outputs with guard rows.  Returns numpy arrays; the pairs (and the segments with them) sorted by (packed query row, target)."""
    dev = device_mesh(target)
    qdev = dev if self_ else device_mesh(query)
    built = run_build(dev, grid) if built is None else built
    QT = qdev["T"]
    m = None if transform is None else torch.from_numpy(np.ascontiguousarray(transform, dtype=F)).cuda()
    out = {"count": poisoned((QT + GUARD,), torch.int32)}
    if "first" in outputs:
        out["first"] = poisoned((QT + GUARD,), torch.int32)
    if "pair_offsets" in outputs:
        out["pair_offsets"] = poisoned((QT + 1 + GUARD,), torch.int32)
    s, workspace, size = call(dev, grid, built, qdev, m, self_, out)
    launch(s, workspace, size)
    torch.cuda.synchronize()
    rows = {"count": QT, "first": QT, "pair_offsets": QT + 1}
    for key, t in out.items():
        assert bool(is_poison(t[rows[key]:]).all()) and not bool(is_poison(t[:rows[key]]).any()), key
    assert bool(is_poison(workspace[size // 4:]).all())
    got = {key: t[:rows[key]].cpu().numpy() for key, t in out.items()}
    got["P"] = int(got["count"].astype(np.int64).sum())
    if "pair_offsets" in got:
        assert got["P"] == int(got["pair_offsets"][QT])
    if "pairs" not in outputs:
        return got
    capacity = got["P"] if capacity is None else capacity
    pairs = poisoned((capacity + GUARD, 2), torch.int32)
    segments = poisoned((capacity + GUARD, 2, 3), torch.float32) if "segments" in outputs else None
    counted = {key: t.clone() for key, t in out.items()}
    s, workspace, size = call(dev, grid, built, qdev, m, self_, out, pairs, segments, capacity)
    launch(s, workspace, size)
    torch.cuda.synchronize()
    for key, t in out.items():
        assert torch.equal(t, counted[key]), key                            # the emitting call reports the same counts and offsets
    written = min(capacity, got["P"])
    for t in (pairs, segments):
        if t is not None:
            assert bool(is_poison(t[written:]).all()) and not bool(is_poison(t[:written]).any())
    assert bool(is_poison(workspace[size // 4:]).all())
    p = pairs[:written].cpu().numpy()
    row = np.searchsorted(np.cumsum(got["count"].astype(np.int64)), np.arange(written), side="right")     # the packed row of every slot
    order = np.lexsort((p[:, 1], row))
    got["pairs"], got["rows"] = p[order], row[order]
    if segments is not None:
        got["segments"] = segments[:written].cpu().numpy()[order]
    return got


def assert_contacts_equal(got, want, what, rows=None):
    """``count``, ``first``, ``pair_offsets``, the sorted pairs and the segments as bits; ``rows``: only the first pairs were emitted."""
    for key in ("count", "first", "pair_offsets"):
        if key in got:
            assert np.array_equal(got[key], want[key]), (what, key, int((got[key] != want[key]).sum()), len(want[key]))
    if "pairs" in got:
        n = len(want["pairs"]) if rows is None else rows
        assert got["pairs"].shape == (n, 2), (what, got["pairs"].shape, n)
        if rows is None:
            assert np.array_equal(got["rows"], want["rows"]) and np.array_equal(got["pairs"], want["pairs"]), what
        else:                                               # a short capacity holds the pairs of the first slots, whole rows first
            whole = want["rows"] < np.searchsorted(want["pair_offsets"][1:], rows, side="right")
            assert np.array_equal(got["pairs"][:int(whole.sum())], want["pairs"][whole]), what
    if "segments" in got and rows is None:
        same = np.all(got["segments"].view(np.int32) == want["segments"].view(np.int32), axis=(1, 2))
        assert same.all(), (what, "segments", int((~same).sum()), len(same), got["segments"][~same][:1], want["segments"][~same][:1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit identity through the C ABI: the grid changes nothing
@pytest.mark.parametrize("grid_name", GRIDS)
@pytest.mark.parametrize("name", ["sphere_shifted", "sphere_torus", "three_groups", "posed", "posed_groups"])
def test_pairs_and_segments_equal_the_exhaustive_rule(name, grid_name):
    target, query, transform = case(name)
    want = reference(name)
    got = run_intersect(target, make_grid(grid_name, AXES[9]), query, transform)
    print(f"{name} {grid_name}: T {target['triangle_offsets'].tolist()}, QT {query['triangle_offsets'].tolist()}, P {got['P']}, "
          f"accepted tests per pair {np.bincount(want['accepted'], minlength=7).tolist()}")
    assert_contacts_equal(got, want, (name, grid_name))
    assert got["P"] == len(want["pairs"]) > 0
    for g in range(len(target["triangle_offsets"]) - 1):
        empty = target["triangle_offsets"][g] == target["triangle_offsets"][g + 1] or query["triangle_offsets"][g] == query["triangle_offsets"][g + 1]
        assert (int((want["groups"] == g).sum()) == 0) == bool(empty)


@pytest.mark.parametrize("grid_name", ["k2", "off_lattice"])
def test_the_lattice_aligned_shift_with_coincident_vertices_and_coplanar_faces(grid_name):
    target, query, _ = case("aligned17")
    want = reference("aligned17")
    got = run_intersect(target, make_grid(grid_name, AXES[17]), query)
    assert_contacts_equal(got, want, ("aligned17", grid_name))
    assert got["P"] == 679 and want["outside_box"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. outputs, capacities, sizes
def test_outputs_in_every_optional_combination():
    target, query, transform = case("three_groups")
    want = reference("three_groups")
    for grid_name in ("k2", "off_lattice"):
        grid = make_grid(grid_name, AXES[9])
        built = run_build(device_mesh(target), grid)
        combinations = [head + tail for head in ((), ("first",), ("pair_offsets",), ("first", "pair_offsets"))
                        for tail in ((), ("pairs",), ("pairs", "segments"))]
        assert len(combinations) == 12 and OUTPUTS in combinations         # segments needs pairs: these are all the valid ones
        for outputs in combinations:
            got = run_intersect(target, grid, query, transform, outputs=outputs, built=built)
            assert ("first" in got) == ("first" in outputs) and ("segments" in got) == ("segments" in outputs)
            assert_contacts_equal(got, want, (grid_name, outputs))


@pytest.mark.parametrize("capacity", [0, 1, 77])
def test_a_short_capacity_writes_nothing_beyond_it(capacity):
    target, query, transform = case("three_groups")
    want = reference("three_groups")
    assert capacity < len(want["pairs"])
    got = run_intersect(target, make_grid("k2", AXES[9]), query, transform, capacity=capacity)
    assert_contacts_equal(got, want, ("capacity", capacity), rows=capacity)


def test_query_counts_that_are_no_multiple_of_256_and_no_query_at_all():
    sphere, torus = part("sphere"), part("torus")
    grid = make_grid("k2", AXES[9])
    for rows in (1, 255, 257, 300):
        cut = ir.packed({"vertices": torus["vertices"], "triangles": torus["triangles"][:rows]})
        query = pack([cut, ir.packed({"vertices": torus["vertices"], "triangles": torus["triangles"][rows:rows + 77]})])
        target = pack([sphere, sphere])
        assert_contacts_equal(run_intersect(target, grid, query), ir.intersect(target, query), ("rows", rows))
    none = pack([EMPTY, EMPTY])
    got = run_intersect(pack([sphere, sphere]), grid, none)
    assert got["P"] == 0 and got["pair_offsets"].tolist() == [0] and got["pairs"].shape == (0, 2)
    got = run_intersect(none, grid, pack([sphere, torus]))                # no target: no reference outside nothing, every count 0
    assert got["P"] == 0 and not got["count"].any() and bool((got["first"] == -1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. hostile input
def test_hostile_targets_queries_and_offsets():
    target, query, _ = case("three_groups")
    transform = np.stack([pose(5.0, (0, 0, 0)), pose(), pose(-5.0, (0.05, 0, 0))])
    bad_t, bad_q = hostile(target), hostile(query, seed=2)
    V, T = len(query["vertices"]), len(query["triangles"])
    moved = dict(bad_q)
    moved["vertex_offsets"] = np.array([-5, query["vertex_offsets"][1], V + 1000, 2 ** 31 - 1], dtype=np.int32)
    moved["triangle_offsets"] = np.array([3, query["triangle_offsets"][1], T - 7, T - 9], dtype=np.int32)     # rows that no group owns
    nan_pose = transform.copy()
    nan_pose[2, 1, 2] = np.nan
    total = 0
    for name, t, q, m in (("target", bad_t, query, None), ("query", target, bad_q, transform), ("both", bad_t, bad_q, transform),
                          ("offsets", bad_t, moved, None), ("nan_transform", target, query, nan_pose)):
        want = ir.intersect(t, q, m)
        total += len(want["pairs"])
        for grid_name in ("k2", "off_lattice"):
            assert_contacts_equal(run_intersect(t, make_grid(grid_name, AXES[9]), q, m), want, (name, grid_name))
        if name == "nan_transform":
            assert int((want["groups"] == 2).sum()) == 0 and int((want["groups"] == 0).sum()) > 0
    assert total > 0


def test_a_stale_grid_costs_correctness_never_memory_safety():
    """The lists of another mesh (and poisoned lists) with this mesh's arrays: guard rows intact, the call returns, and every pair it
    reports is a pair of the rule."""
    target, query, transform = case("three_groups")
    want = reference("three_groups")
    known = set(map(tuple, np.column_stack([want["rows"], want["pairs"][:, 1]]).tolist()))
    grid = make_grid("k2", AXES[9])
    other = pack([part("torus"), part("sphere"), EMPTY])
    dev = device_mesh(target)
    stale = (run_build(device_mesh(other), grid), run_build(device_mesh(hostile(other)), grid),
             (poisoned((lists_of(dev, grid) + 1,), torch.int32), poisoned((64,), torch.int32), 64))
    for built in stale:
        got = run_intersect(target, grid, query, transform, built=built)
        assert set(map(tuple, np.column_stack([got["rows"], got["pairs"][:, 1]]).tolist())) <= known


# ---------------------------------------------------------------------------------------------------------------------
# 4. self mode
def simplified_off_lattice():
    field, axes = sr.sphere_field(17)
    return ir.packed(sp.simplify_mesh(sr.extract_surface(field[None], axes, 0.0), *OFF_LATTICE))


def test_self_mode():
    grid = make_grid("k2", AXES[9])
    for kind in ("sphere", "torus"):
        got = run_intersect(part(kind), grid, self_=True)
        assert got["P"] == 0 and bool((got["first"] == -1).all()), kind                 # a clean mesh does not cut itself
    sphere = part("sphere")
    two = ir.joined(sphere, ir.shifted(sphere, SHIFT))
    want = ir.intersect(two, self_=True)
    assert len(want["pairs"]) == 2 * len(reference("sphere_shifted")["pairs"])          # every unordered pair from both sides
    for grid_name in ("k2", "off_lattice", "one_cell"):
        assert_contacts_equal(run_intersect(two, make_grid(grid_name, AXES[9]), self_=True), want, ("two spheres", grid_name))
    mesh = simplified_off_lattice()
    want = ir.intersect(mesh, self_=True)
    print(f"sphere 17^3 simplified on the off-lattice grid: T {len(mesh['triangles'])}, self pairs {len(want['pairs'])}")
    for grid_name in ("k2", "off_lattice"):
        assert_contacts_equal(run_intersect(mesh, make_grid(grid_name, AXES[17]), self_=True), want, ("simplified", grid_name))
    groups = pack([two, EMPTY, part("torus")])
    assert_contacts_equal(run_intersect(groups, grid, self_=True), ir.intersect(groups, self_=True), "self, three groups")


# ---------------------------------------------------------------------------------------------------------------------
# 5. repeated and recorded calls
def test_the_same_call_twice_and_a_grid_built_twice_give_equal_results():
    """The lists fill in the order of arrival, which differs from build to build; the sorted result must not."""
    target, query, transform = case("posed_groups")
    grid = make_grid("k4", AXES[9])
    dev = device_mesh(target)
    first, second = run_build(dev, grid), run_build(dev, grid)
    a, b, c = (run_intersect(target, grid, query, transform, built=built) for built in (first, first, second))
    for key in ("count", "first", "pair_offsets", "pairs"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
    assert np.array_equal(a["segments"].view(np.int32), b["segments"].view(np.int32))
    assert np.array_equal(a["segments"].view(np.int32), c["segments"].view(np.int32))


def test_recorded_call_is_kernels_only_and_replays_on_another_pose():
    target, query, _ = case("posed")
    want = reference("posed")
    other = pose(-60.0, (0.0, 0.25, 0.1))[None]
    want_other = ir.intersect(target, query, other)
    grid = make_grid("k2", AXES[9])
    dev, qdev = device_mesh(target), device_mesh(query)
    built = run_build(dev, grid)
    QT, capacity = qdev["T"], max(len(want["pairs"]), len(want_other["pairs"]))
    m = torch.zeros((1, 3, 4), device="cuda")
    out = {"count": poisoned((QT + GUARD,), torch.int32), "first": poisoned((QT + GUARD,), torch.int32),
           "pair_offsets": poisoned((QT + 1 + GUARD,), torch.int32)}
    pairs, segments = poisoned((capacity + GUARD, 2), torch.int32), poisoned((capacity + GUARD, 2, 3), torch.float32)
    s, workspace, size = call(dev, grid, built, qdev, m, False, out, pairs, segments, capacity)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(s, workspace, size)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        launch(s, workspace, size)
    census = frame_graph.node_census(graph)
    graph.instantiate()
    print("recorded call:", census)
    assert census == {"nodes": 6, "kernels": 6, "memsets": 0, "memcpys": 0}
    for matrix, expect in ((other, want_other), (pose()[None], want), (other, want_other)):
        m.copy_(torch.from_numpy(matrix))
        for t in list(out.values()) + [pairs, segments]:
            t.view(torch.int32).fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        P = len(expect["pairs"])
        assert np.array_equal(out["count"][:QT].cpu().numpy(), expect["count"]) and np.array_equal(out["first"][:QT].cpu().numpy(), expect["first"])
        offsets = out["pair_offsets"][:QT + 1].cpu().numpy()
        assert np.array_equal(offsets, expect["pair_offsets"])
        p = pairs[:P].cpu().numpy()
        row = np.searchsorted(offsets[1:], np.arange(P), side="right")
        order = np.lexsort((p[:, 1], row))
        assert np.array_equal(p[order], expect["pairs"])
        assert np.array_equal(segments[:P].cpu().numpy()[order].view(np.int32), expect["segments"].view(np.int32))
        assert bool(is_poison(pairs[P:]).all()) and bool(is_poison(segments[P:]).all())
        assert all(bool(is_poison(t[n:]).all()) for t, n in ((out["count"], QT), (out["first"], QT), (out["pair_offsets"], QT + 1)))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the python layer
def contacts_dict(contacts):
    out = {"count": contacts.count.cpu().numpy(), "first": contacts.first.cpu().numpy(), "pair_offsets": contacts.offsets.cpu().numpy()}
    if contacts.pairs is not None:
        out["pairs"] = contacts.pairs.cpu().numpy()
    if contacts.segments is not None:
        out["segments"] = contacts.segments.cpu().numpy()
    return out


def group_of(want, g, query):
    """The reference's result restricted to group g, with the offsets of that group alone."""
    to = query["triangle_offsets"]
    own = want["groups"] == g
    count = want["count"][to[g]:to[g + 1]]
    return {"count": count, "first": want["first"][to[g]:to[g + 1]], "pair_offsets": np.concatenate([[0], np.cumsum(count)]).astype(np.int32),
            "pairs": want["pairs"][own], "rows": want["rows"][own] - to[g], "segments": want["segments"][own]}


def test_ray_grid_intersect_mesh_intersections_and_self_intersections():
    target, query, transform = case("posed_groups")
    want = reference("posed_groups")
    targets, queries = to_meshes(target), to_meshes(query)
    grid = surface.RayGrid.build(targets, *surface.bounding_grid([m for m in targets if m.vertices.numel()], (12, 16, 20)))
    m = torch.from_numpy(transform).cuda()
    found = grid.intersect(queries, transform=m, pairs=True, segments=True)
    assert len(found) == 3
    for g, contacts in enumerate(found):
        got = contacts_dict(contacts)
        got["rows"] = got["pairs"][:, 0].astype(np.int64)
        assert_contacts_equal(got, group_of(want, g, query), ("RayGrid.intersect", g))
        report = contacts.report()
        own = want["groups"] == g
        assert report["pairs"] == int(own.sum()) and report["intersecting"] == bool(own.any())
        assert report["query_triangles"] == len(np.unique(want["rows"][own])) and report["target_triangles"] == len(np.unique(want["pairs"][own, 1]))
        s = want["segments"][own].astype(np.float64)
        assert math.isclose(report["contact_length"], float(np.linalg.norm(s[:, 1] - s[:, 0], axis=1).sum()), rel_tol=1e-12, abs_tol=1e-12)
    bare = grid.intersect(queries, transform=m)
    assert all(b.pairs is None and b.segments is None and torch.equal(b.count, f.count) and torch.equal(b.first, f.first)
               for b, f in zip(bare, found))
    assert bare[0].report()["target_triangles"] is None and bare[0].report()["contact_length"] is None
    # one (4, 4) matrix for every group, and Mesh.intersections against a mesh and against a grid of one group
    four = torch.cat([m[0], torch.tensor([[0.0, 0.0, 0.0, 1.0]], device="cuda")])
    sphere, torus = to_meshes(pack([part("sphere"), part("torus")]))
    want_one = group_of(reference("posed"), 0, case("posed")[1])
    for other in (sphere, sphere.ray_grid(*make_grid("off_lattice", AXES[9]))):
        got = contacts_dict(torus.intersections(other, transform=four, pairs=True, segments=True, cells=8))
        got["rows"] = got["pairs"][:, 0].astype(np.int64)
        assert_contacts_equal(got, want_one, "Mesh.intersections")
    # self-intersections: none on the clean meshes, the reference's on two spheres in one mesh
    assert sphere.self_intersections(cells=8).report() == {"pairs": 0, "query_triangles": 0, "target_triangles": None, "contact_length": None,
                                                           "intersecting": False}
    two = ir.joined(part("sphere"), ir.shifted(part("sphere"), SHIFT))
    both = to_meshes(two)[0].self_intersections(cells=16, pairs=True)
    want_two = ir.intersect(two, self_=True)
    assert np.array_equal(both.pairs.cpu().numpy(), want_two["pairs"]) and both.symmetric
    assert both.report()["pairs"] == len(reference("sphere_shifted")["pairs"]) and both.report()["intersecting"]
    for bad in (lambda: grid.intersect(queries[:2]), lambda: grid.intersect(queries, transform=m[:2]),
                lambda: grid.intersect(queries, self_=True), lambda: grid.intersect(self_=True, transform=m),
                lambda: torus.intersections(grid), lambda: grid.intersect(queries, transform=torch.zeros(3, 3, 3))):
        with pytest.raises(ValueError):
            bad()


def test_collide_on_disjoint_touching_and_nested_spheres():
    sphere = to_meshes(part("sphere"))[0]
    move = lambda x, scale=1.0: torch.tensor([[scale, 0, 0, x], [0, scale, 0, 0], [0, 0, scale, 0]], dtype=torch.float32)
    shifted = lambda x, scale=1.0: ir.intersect(part("sphere"), part("sphere"), move(x, scale).numpy()[None])
    apart = surface.collide(sphere, sphere, transform=move(2.0), inside=True)
    assert (apart.intersecting, apart.pairs, apart.b_in_a) == (False, 0, False)
    want = shifted(1.2)                                                    # 2 r = 1.26: the surfaces touch in a small circle
    touching = surface.collide(sphere, sphere, transform=move(1.2), cells=8)
    assert touching.intersecting and touching.pairs == len(want["pairs"]) > 0 and touching.b_in_a is None
    nested = surface.collide(sphere, sphere, transform=move(0.05, 0.5), inside=True)
    assert len(shifted(0.05, 0.5)["pairs"]) == 0
    assert (nested.intersecting, nested.pairs, nested.b_in_a) == (False, 0, True)          # swallowed whole: only `inside` sees it
    grid = sphere.ray_grid(*make_grid("k2", AXES[9]))                      # a static object's grid, built once
    cut = surface.collide(grid, sphere, transform=move(0.3), inside=True)
    assert cut.intersecting and cut.pairs == len(shifted(0.3)["pairs"]) and cut.b_in_a in (True, False)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the composer
def test_the_composers_meshes_against_each_other_and_themselves():
    """``extract_mesh`` of the small tennis ``player_1`` network on a 12^3 lattice: every eighth triangle of one style's mesh, posed,
    against the whole mesh of the other style, on the lattice's cluster grid and on a bounding grid; and the first thousand triangles
    of a mesh against themselves.  (The exhaustive reference, not the call, is what the sizes are cut for.)"""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 12, style, deformation)
        meshes = comp.extract_mesh(PLAYER_1, 12, style, deformation, level=float(sigma.median()))
    queries = [Mesh(m.vertices, m.triangles[::8].contiguous()) for m in meshes[::-1]]
    as_dict = lambda ms: pack([{"vertices": m.vertices.cpu().numpy(), "triangles": m.triangles.cpu().numpy()} for m in ms])
    target, query = as_dict(meshes), as_dict(queries)
    assert target["triangle_offsets"][1] > 0 and target["triangle_offsets"][2] > target["triangle_offsets"][1]
    extent = float(np.ptp(target["vertices"], axis=0).max())
    transform = np.stack([pose(10.0, (0.02 * extent, 0, 0)), pose(-15.0, (0, 0.03 * extent, 0))])
    want = ir.intersect(target, query, transform)
    axes = [centres[:, 0, 0, 0].cpu().numpy(), centres[0, :, 0, 1].cpu().numpy(), centres[0, 0, :, 2].cpu().numpy()]
    for grid in (surface.lattice_cluster_grid(axes, 2), surface.bounding_grid(meshes, 16)):
        found = surface.RayGrid.build(meshes, *grid).intersect(queries, transform=torch.from_numpy(transform).cuda(), pairs=True, segments=True)
        for g, contacts in enumerate(found):
            got = contacts_dict(contacts)
            got["rows"] = got["pairs"][:, 0].astype(np.int64)
            assert_contacts_equal(got, group_of(want, g, query), ("composer", g))
    print(f"composer: T {target['triangle_offsets'].tolist()}, QT {query['triangle_offsets'].tolist()}, pairs {len(want['pairs'])}")
    assert len(want["pairs"]) > 0
    piece = Mesh(meshes[0].vertices, meshes[0].triangles[:1000].contiguous())
    own = ir.intersect(as_dict([piece]), self_=True)
    found = piece.self_intersections(cells=16, pairs=True)
    assert np.array_equal(found.pairs.cpu().numpy(), own["pairs"]) and np.array_equal(found.count.cpu().numpy(), own["count"])

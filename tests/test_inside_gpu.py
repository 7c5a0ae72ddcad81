"""Inside / outside queries on the GPU (python -m pytest tests -m gpu): ``pr_inside_query`` against the exhaustive numpy sum
(tests/inside_reference.py) - ``winding`` and ``crossings`` as integers for every point of every set, on every mesh, in one and three
groups, on seven grids and all three axes; poisoned outputs with guard rows, hostile and stale input, repeated and recorded calls; the
Python layer and ``ObjectComposer.extract_mesh`` on the small tennis networks.  The reference does not depend on the grid, so one
result per (mesh, groups, axis) serves all grids.  There is no domain restriction: the sets 2^12 cells away and outside the grid's
box are compared like every other."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, surface
from tests import components_reference as cc
from tests import inside_reference as ir
from tests import surface_reference as sr
from tests.test_raycast_gpu import device_mesh, hostile, lists_of, run_build, to_meshes
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, make_field, poisoned, tennis

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes, points, references (numpy only)
_CASES = {}


def make_batch(mesh, axes, n, seed=0):
    return ir.point_batch(mesh, axes, n, [ir.make_grid("k2", axes, mesh), ir.OFF_LATTICE], seed)


def case(kind, groups):
    """(mesh, axes, points, sets, [reference result per axis]) - computed once per (mesh, groups)."""
    key = (kind, groups)
    if key not in _CASES:
        mesh, axes = ir.mesh_case(kind, groups)
        points, sets = make_batch(mesh, axes, ir.points_per_set(mesh))
        _CASES[key] = (mesh, axes, points, sets, [ir.rule(mesh, points, axis) for axis in range(3)])
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def run_inside(dev, grid, built, points, axis, crossings=True):
    """One call on poisoned outputs with guard rows."""
    cell_offsets, references, R = built
    G, N = points.shape[:2]
    p = torch.from_numpy(np.ascontiguousarray(points)).cuda()
    out = {"winding": poisoned((G * N + GUARD,), torch.int32)}
    if crossings:
        out["crossings"] = poisoned((G * N + GUARD,), torch.int32)
    s = surface.inside_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                              cell_offsets, references=references[:R] if R else None, points=p, axis=axis, **out)
    _lib.check(_lib.load().pr_inside_query(C.byref(s), torch.cuda.current_stream().cuda_stream), "pr_inside_query")
    torch.cuda.synchronize()
    for key, t in out.items():
        assert bool(is_poison(t[G * N:]).all()), key
    return {key: t[:G * N].reshape(G, N) for key, t in out.items()}


def assert_inside_equal(got, want, what, sets=None):
    """Every point: ``winding`` and ``crossings`` as integers."""
    got = {key: t.cpu().numpy() for key, t in got.items()}
    same = np.ones(want["winding"].shape, dtype=bool)
    for key in got:
        same &= got[key] == want[key]
    if not same.all():
        g, r = np.argwhere(~same)[0]
        name = [k for k, sl in (sets or {}).items() if sl.start <= r < sl.stop]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} points differ; first: group {g} point {r} {name}: got "
                             f"{ {k: int(v[g, r]) for k, v in got.items()} }, want winding {int(want['winding'][g, r])} crossings "
                             f"{int(want['crossings'][g, r])}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. integer identity through the C ABI
@pytest.mark.parametrize("grid_name", ir.GRIDS)
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", ir.MESHES)
def test_windings_equal_the_exhaustive_sum(kind, groups, grid_name):
    mesh, axes, points, sets, wants = case(kind, groups)
    grid = ir.make_grid(grid_name, axes, mesh)
    dev = device_mesh(mesh)
    built = run_build(dev, grid)
    for axis, want in enumerate(wants):
        got = run_inside(dev, grid, built, points, axis)
        assert_inside_equal(got, want, (kind, groups, grid_name, axis), sets)
        assert not want["winding"][:, sets["not_finite"]].any() and not want["crossings"][:, sets["not_finite"]].any()
        assert int(want["crossings"].sum()) > 0
        if kind in ir.BALANCED:
            assert not want["coverage"].any()
    print(f"{kind} G={groups} {grid_name}: T {mesh['triangle_offsets'].tolist()}, R {built[2]}, points {points.shape[1]} per group, inside "
          f"{[int((w['winding'] != 0).sum()) for w in wants]}, crossings {[int(w['crossings'].sum()) for w in wants]}")


def test_crossings_are_optional():
    mesh, axes, points, sets, wants = case("sphere", 3)
    dev = device_mesh(mesh)
    for grid_name in ("k2", "off_lattice"):
        grid = ir.make_grid(grid_name, axes, mesh)
        built = run_build(dev, grid)
        for axis in range(3):
            got = run_inside(dev, grid, built, points, axis, crossings=False)
            assert set(got) == {"winding"}
            assert_inside_equal(got, wants[axis], (grid_name, axis), sets)


@pytest.mark.parametrize("count", [1, 77])
def test_one_point_and_a_count_that_is_no_multiple_of_64(count):
    mesh, axes, points, sets, wants = case("torus", 3)
    pick = np.linspace(0, points.shape[1] - 1, count).astype(np.int64)
    grid = ir.make_grid("k2", axes, mesh)
    dev = device_mesh(mesh)
    built = run_build(dev, grid)
    for axis in range(3):
        want = {key: wants[axis][key][:, pick] for key in ("winding", "crossings")}
        assert_inside_equal(run_inside(dev, grid, built, points[:, pick], axis), want, (count, axis))


def test_five_groups_with_empty_meshes_between_and_an_empty_mesh():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    parts = []
    for g, kind in enumerate(["torus", "all_outside", "noise", "all_inside", "sphere"]):
        field, level = make_field(kind, shape, axes, seed=50 + g)
        parts.append(sr.extract_surface(field[None], axes, level))
    mesh = ir.pack(parts)
    to = mesh["triangle_offsets"].tolist()
    assert to[1] == to[2] and to[3] == to[4] and to[0] < to[1] < to[3] < to[5]
    points, sets = make_batch(mesh, axes, 12)
    dev = device_mesh(mesh)
    for axis in range(3):
        want = ir.rule(mesh, points, axis)
        for grid_name in ("k2", "off_lattice"):
            grid = ir.make_grid(grid_name, axes, mesh)
            assert_inside_equal(run_inside(dev, grid, run_build(dev, grid), points, axis), want, ("five groups", grid_name, axis), sets)
        assert not want["crossings"][1].any() and not want["crossings"][3].any() and want["crossings"][0].any() and want["crossings"][4].any()
    # an entirely empty mesh: zeros
    empty = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32), "vertex_offsets": np.zeros(3, np.int32),
             "triangle_offsets": np.zeros(3, np.int32)}
    dev = device_mesh(empty)
    grid = ir.make_grid("k2", axes, mesh)
    built = run_build(dev, grid)
    assert built[2] == 0
    for axis in range(3):
        got = run_inside(dev, grid, built, points[:2], axis)
        assert not bool(got["winding"].any()) and not bool(got["crossings"].any())


def test_hostile_meshes_and_offsets():
    mesh, axes, points, sets, _ = case("sphere", 3)
    bad = hostile(mesh)
    V, T = len(mesh["vertices"]), len(mesh["triangles"])
    cases = [("values", bad)]
    for name, vo, to in (("decreasing", [0, mesh["vertex_offsets"][2], mesh["vertex_offsets"][1], V], [0, mesh["triangle_offsets"][2], mesh["triangle_offsets"][1], T]),
                         ("leaving", [-5, mesh["vertex_offsets"][1], V + 1000, 2 ** 31 - 1], [-2 ** 31, mesh["triangle_offsets"][1], T + 7, T + 9])):
        changed = dict(bad)
        changed["vertex_offsets"], changed["triangle_offsets"] = np.array(vo, dtype=np.int32), np.array(to, dtype=np.int32)
        cases.append((name, changed))
    for name, changed in cases:
        dev = device_mesh(changed)
        for axis in range(3):
            want = ir.rule(changed, points, axis)
            for grid_name in ("k2", "off_lattice"):
                grid = ir.make_grid(grid_name, axes, mesh)
                got = run_inside(dev, grid, run_build(dev, grid), points, axis)
                assert_inside_equal(got, want, (name, grid_name, axis), sets)
            assert int(want["crossings"].sum()) > 0


def test_a_stale_grid_costs_correctness_never_memory_safety():
    """The lists of another mesh (and of a hostile one, and poisoned lists) with this mesh's arrays: the guard rows stay intact and the
    call returns."""
    mesh, axes, points, sets, _ = case("sphere", 3)
    other, _ = ir.mesh_case("noise", 3)
    grid = ir.make_grid("k2", axes, mesh)
    dev = device_mesh(mesh)
    for source in (other, hostile(other)):
        built = run_build(device_mesh(source), grid)
        for axis in range(3):
            run_inside(dev, grid, built, points, axis)
    poisoned_lists = (poisoned((lists_of(dev, grid) + 1,), torch.int32), poisoned((64,), torch.int32), 64)
    for axis in range(3):
        run_inside(dev, grid, poisoned_lists, points, axis)


def test_the_same_call_twice_and_a_grid_built_twice_give_equal_results():
    """The lists fill in the order of arrival, which differs from build to build; a sum of integers does not depend on it."""
    mesh, axes, points, sets, wants = case("noise", 1)
    grid = ir.make_grid("k4", axes, mesh)
    dev = device_mesh(mesh)
    first, second = run_build(dev, grid), run_build(dev, grid)
    for axis in range(3):
        a, b, c = run_inside(dev, grid, first, points, axis), run_inside(dev, grid, first, points, axis), run_inside(dev, grid, second, points, axis)
        for key in a:
            assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]), (axis, key)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a recorded call
def test_recorded_query_is_one_kernel_and_replays_on_another_mesh_and_other_points():
    mesh, axes, points, sets, wants = case("sphere", 3)
    second, _ = ir.mesh_case("torus", 3)
    other, _ = make_batch(second, axes, ir.points_per_set(second), seed=1)
    grid = ir.make_grid("k2", axes, mesh)
    axis = 1
    devs = [device_mesh(mesh), device_mesh(second)]
    builts = [run_build(dev, grid) for dev in devs]
    # one set of buffers that holds either mesh: the totals the call is told are the capacities, the offsets say what is there
    V, T, R = max(d["V"] for d in devs), max(d["T"] for d in devs), max(b[2] for b in builts)
    G, N = points.shape[:2]
    held = {"vertices": torch.zeros((V, 3), device="cuda"), "triangles": torch.zeros((T, 3), dtype=torch.int32, device="cuda"),
            "vertex_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda"), "triangle_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda"),
            "cell_offsets": torch.zeros(lists_of(devs[0], grid) + 1, dtype=torch.int32, device="cuda"),
            "references": torch.zeros(R, dtype=torch.int32, device="cuda")}

    def load(which):
        dev, (cell_offsets, references, r) = devs[which], builts[which]
        held["vertices"][:dev["V"]].copy_(dev["vertices"][:dev["V"]])
        held["triangles"][:dev["T"]].copy_(dev["triangles"][:dev["T"]])
        held["vertex_offsets"].copy_(dev["vertex_offsets"])
        held["triangle_offsets"].copy_(dev["triangle_offsets"])
        held["cell_offsets"].copy_(cell_offsets[:held["cell_offsets"].numel()])
        held["references"][:r].copy_(references[:r])

    load(0)
    p = torch.zeros((G, N, 3), device="cuda")
    out = {"winding": poisoned((G * N + GUARD,), torch.int32), "crossings": poisoned((G * N + GUARD,), torch.int32)}
    s = surface.inside_struct(held["vertices"], held["triangles"], held["vertex_offsets"], held["triangle_offsets"], V, T, *grid,
                              held["cell_offsets"], references=held["references"], points=p, axis=axis, **out)
    lib = _lib.load()
    call = lambda: _lib.check(lib.pr_inside_query(C.byref(s), torch.cuda.current_stream().cuda_stream), "pr_inside_query")
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
    print("recorded query:", census)
    assert census == {"nodes": 1, "kernels": 1, "memsets": 0, "memcpys": 0}
    for which, batch, want in ((0, points, wants[axis]), (1, other, ir.rule(second, other, axis)), (0, other, ir.rule(mesh, other, axis))):
        load(which)
        p.copy_(torch.from_numpy(batch))
        for t in out.values():
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        got = {key: t[:G * N].reshape(G, N) for key, t in out.items()}
        assert_inside_equal(got, want, ("replay", which), sets)
        assert all(bool(is_poison(t[G * N:]).all()) for t in out.values())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the python layer
def test_ray_grid_winding_contains_and_signed_distance():
    mesh, axes, points, sets, wants = case("sphere", 3)
    meshes = to_meshes(mesh)
    grid = surface.RayGrid.build(meshes, *surface.bounding_grid(meshes, (12, 16, 20)))
    to_cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = to_cuda(points)
    for axis in range(3):
        found = grid.winding(p, axis=axis, crossings=True)
        assert found.winding.dtype == torch.int32 and found.crossings.dtype == torch.int32
        assert_inside_equal({"winding": found.winding, "crossings": found.crossings}, wants[axis], ("RayGrid.winding", axis), sets)
        bare = grid.winding(p, axis=axis)
        assert bare.crossings is None and torch.equal(bare.winding, found.winding)
        inside = grid.contains(p, axis=axis)
        assert inside.dtype == torch.bool and torch.equal(inside, found.winding != 0)
        each, anywhere, lowest = grid.contains(p, axis=axis, any=True)
        assert torch.equal(each, inside) and torch.equal(anywhere, inside.any(dim=0)) and lowest.dtype == torch.int64
        first = torch.where(inside[0], 0, torch.where(inside[1], 1, torch.where(inside[2], 2, -1)))
        assert torch.equal(lowest, first)
        assert int((lowest >= 0).sum()) > 0 and int((lowest < 0).sum()) > 0
    assert torch.equal(grid.winding(p).winding, grid.winding(p, axis=2).winding)                       # the default axis
    radius = 0.25
    distance = grid.closest(p, max_distance=radius).distance
    inside = grid.contains(p)
    signed = grid.signed_distance(p, max_distance=radius)
    assert torch.equal(signed, torch.where(inside, -distance, distance))
    assert bool((signed == -math.inf).any()) and bool((signed == math.inf).any()) and bool(((signed < 0) & (signed > -math.inf)).any())
    assert torch.equal(grid.signed_distance(p, max_distance=radius, nearest=True), signed.amin(dim=0))
    assert torch.equal(grid.signed_distance(p, max_distance=radius, axis=0), torch.where(grid.contains(p, axis=0), -distance, distance))
    # (N, 3) points are used for every group
    shared = grid.winding(p[0], axis=1, crossings=True)
    want = ir.rule(mesh, np.broadcast_to(points[:1], points.shape).copy(), 1)
    assert_inside_equal({"winding": shared.winding, "crossings": shared.crossings}, want, "shared points")
    assert list(grid.winding(p[:, :0]).winding.shape) == [3, 0] and list(grid.contains(p[:, :0]).shape) == [3, 0]
    for bad in (lambda: grid.winding(p[:2]), lambda: grid.winding(p[..., :2]), lambda: grid.winding(p, axis=3), lambda: grid.winding(p, axis=-1),
                lambda: grid.winding(p, axis=1.5), lambda: grid.contains(p, axis=3), lambda: grid.signed_distance(p, max_distance=math.nan),
                lambda: grid.signed_distance(p, max_distance=1.0, axis=7)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        grid.signed_distance(p)                                           # max_distance has no default


# ---------------------------------------------------------------------------------------------------------------------
# 4. the composer
def test_contains_at_the_lattice_points_is_the_lattices_own_inside_mask():
    """``extract_mesh(close_border=True)`` of the small tennis ``player_1`` network at resolution 24, level = the median: ``contains``
    at the lattice centres equals the inside mask of the cleaned lattice (the border counts as outside) at every lattice point whose
    value there is not the level, on all three axes, without exception."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        meshes = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, close_border=True)
    cleaned = cc.clean(sigma.cpu().numpy(), level, close_border=True)["sigma_out"]
    decided = torch.from_numpy(cleaned != F(level)).cuda().reshape(len(meshes), -1)
    want = torch.from_numpy(cc.inside_mask(sigma.cpu().numpy(), level, close_border=True)).cuda().reshape(len(meshes), -1)
    assert int(decided.sum()) > decided.numel() // 2 and 0 < int(want.sum()) < want.numel()
    points = centres.reshape(-1, 3)
    for cells in (16, (5, 9, 24)):
        grid = surface.RayGrid.build(meshes, *surface.bounding_grid(meshes, cells))
        for axis in range(3):
            got = grid.contains(points, axis=axis)
            wrong = (got != want) & decided
            print(f"cells {cells} axis {axis}: T {[m.triangles.size(0) for m in meshes]}, inside {int(got.sum())} of {got.numel()}, compared "
                  f"{int(decided.sum())}, wrong {int(wrong.sum())}")
            assert not bool(wrong.any()), (cells, axis, int(wrong.sum()))


def test_contains_on_the_composers_simplified_mesh_equals_the_reference():
    """The same with ``simplify=2, keep_duplicates=True``: against the numpy sum on the call's own mesh, every lattice point."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        meshes = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, close_border=True, simplify=2, keep_duplicates=True)
        removed = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, close_border=True, simplify=2)
    assert all(m.triangles.size(0) >= r.triangles.size(0) for m, r in zip(meshes, removed))
    mesh = ir.pack([{"vertices": m.vertices.cpu().numpy(), "triangles": m.triangles.cpu().numpy()} for m in meshes])
    assert ir.directed_edges_balanced(mesh) and mesh["triangle_offsets"][1] > 0
    points = centres.reshape(-1, 3)
    host = np.broadcast_to(points.cpu().numpy()[None], (len(meshes),) + tuple(points.shape)).copy()
    grid = surface.RayGrid.build(meshes, *surface.bounding_grid(meshes, 16))
    for axis in range(3):
        want = ir.rule(mesh, host, axis)
        found = grid.winding(points, axis=axis, crossings=True)
        assert_inside_equal({"winding": found.winding, "crossings": found.crossings}, want, ("composer, simplified", axis))
        assert not want["coverage"].any()
        assert torch.equal(grid.contains(points, axis=axis), torch.from_numpy(want["winding"] != 0).cuda())
    print(f"simplified: T {mesh['triangle_offsets'].tolist()} (duplicates removed: {[r.triangles.size(0) for r in removed]}), inside "
          f"{int((want['winding'] != 0).sum())} of {want['winding'].size}")

"""Closest-point queries on the GPU (python -m pytest tests -m gpu): ``pr_closest_query`` against the exhaustive numpy search
(tests/closest_reference.py) bit for bit - ``distance`` as bits, ``triangle``, ``point`` and ``barycentric`` as bits - for every point
of every set, on the meshes and grids of tests/test_raycast_gpu.py in one and three groups, at four radii; poisoned outputs with guard
rows, every optional combination of outputs, hostile and stale input, repeated and recorded calls; the Python layer and
``ObjectComposer.extract_mesh`` on the small tennis networks.  The reference does not depend on the grid, so one table of (point,
triangle) pairs per (mesh, point batch) serves all grids and radii.  The set "beyond" lies outside the domain of the guarantee: it is
checked for memory safety, termination and - in float64 - for being an accepted candidate of the rule, not for bits."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, frame_graph, surface
from tests import closest_reference as cr
from tests import raycast_reference as rr
from tests import surface_reference as sr
from tests.test_raycast_gpu import (GRIDS, MESHES, device_mesh, hostile, lists_of, make_grid, mesh_case, pack, run_build, to_meshes)
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, make_field, poisoned, tennis

pytestmark = pytest.mark.gpu

F = np.float32
OUTPUTS = ("distance", "triangle", "point", "barycentric")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes, grids, points, radii (numpy only: nothing here needs a GPU)
def steps(axes):
    """(the smallest cell of the k = 2 lattice grid - "a cell" of the point sets and radii -, the smallest cell of all five grids)."""
    smallest = [float(np.min(np.asarray(make_grid(name, axes)[1], dtype=np.float64))) for name in GRIDS]
    return smallest[GRIDS.index("k2")], min(smallest)


def radii(axes):
    """inf, 0, half a cell, and one cell - which splits the sets on cell faces and corners into hits and misses
    (tests/test_closest_cpu.py checks that on the sphere)."""
    step, _ = steps(axes)
    return [math.inf, 0.0, 0.5 * step, 1.0 * step]


def points_per_set(mesh):
    return 16 if mesh["triangle_offsets"][-1] < 12000 else 4                # (12 sets: 192 points, 48 for the large meshes)


def make_batch(mesh, axes, n, seed=0):
    step, finest = steps(axes)
    return cr.point_batch(mesh, axes, n, [make_grid("k2", axes), make_grid("off_lattice", axes)], finest, seed)


_BATCH, _WANT = {}, {}


def case(kind, groups):
    """(mesh, axes, points, sets, {radius: reference result}) - computed once per (mesh, groups); the table of pairs is dropped."""
    key = (kind, groups)
    if key not in _BATCH:
        mesh, axes, _ = mesh_case(kind, groups)
        points, sets = make_batch(mesh, axes, points_per_set(mesh))
        tables = cr.pair_table(mesh, points)
        _BATCH[key] = (mesh, axes, points, sets)
        _WANT[key] = {r: cr.closest(mesh, points, r, tables) for r in radii(axes)}
    return _BATCH[key] + (_WANT[key],)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def run_closest(dev, grid, built, points, max_distance, outputs=OUTPUTS, rows=None):
    """One call on poisoned outputs with guard rows; ``outputs``: which of the four the call is given."""
    cell_offsets, references, R = built
    G, N = points.shape[:2]
    p = torch.from_numpy(np.ascontiguousarray(points)).cuda()
    shapes = {"distance": ((G * N + GUARD,), torch.float32), "triangle": ((G * N + GUARD,), torch.int32),
              "point": ((G * N + GUARD, 3), torch.float32), "barycentric": ((G * N + GUARD, 2), torch.float32)}
    out = {key: poisoned(*shapes[key]) for key in outputs}
    s = surface.closest_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                               cell_offsets, references=references[:R] if R else None, points=p, max_distance=max_distance, **out)
    _lib.check(_lib.load().pr_closest_query(C.byref(s), torch.cuda.current_stream().cuda_stream), "pr_closest_query")
    torch.cuda.synchronize()
    for key, t in out.items():
        assert bool(is_poison(t[G * N:]).all()), key
    return {key: t[:G * N].reshape((G, N) + tuple(t.shape[1:])) for key, t in out.items()}


def to_numpy(got):
    return {key: t.cpu().numpy() for key, t in got.items()}


def assert_closest_equal(got, want, what, sets=None, skip=None):
    """Every point (but the slice ``skip``): ``distance`` as bits, ``triangle``, ``point`` and ``barycentric`` as bits."""
    got = to_numpy(got)
    same = got["distance"].view(np.int32) == want["distance"].view(np.int32)
    if "triangle" in got:
        same &= got["triangle"] == want["triangle"]
    for key in ("point", "barycentric"):
        if key in got:
            same &= np.all(got[key].view(np.int32) == want[key].view(np.int32), axis=-1)
    if skip is not None:
        same[:, skip] = True
    if not same.all():
        g, r = np.argwhere(~same)[0]
        name = [k for k, sl in (sets or {}).items() if sl.start <= r < sl.stop]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} points differ; first: group {g} point {r} {name}: got distance "
                             f"{got['distance'][g, r]!r} triangle {int(got['triangle'][g, r]) if 'triangle' in got else None}, want distance "
                             f"{want['distance'][g, r]!r} triangle {int(want['triangle'][g, r])}")


def assert_candidates(mesh, points, got, max_distance, rows=None):
    """The float64 "is an accepted candidate" check of the results (no optimality): what holds outside the domain too."""
    cr.check_float64(mesh, points, to_numpy(got), max_distance, optimal=False, rows=rows)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit identity through the C ABI
@pytest.mark.parametrize("grid_name", GRIDS)
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", MESHES)
def test_closest_points_equal_the_exhaustive_search(kind, groups, grid_name):
    mesh, axes, points, sets, wants = case(kind, groups)
    grid = make_grid(grid_name, axes)
    dev = device_mesh(mesh)
    built = run_build(dev, grid)
    for radius, want in wants.items():
        got = run_closest(dev, grid, built, points, radius)
        assert_closest_equal(got, want, (kind, groups, grid_name, radius), sets, skip=sets["beyond"])
        assert_candidates(mesh, points, got, radius, rows=sets["beyond"])
        assert int((want["triangle"][:, sets["not_finite"]] >= 0).sum()) == 0
    hits = {r: int((w["triangle"] >= 0).sum()) for r, w in wants.items()}
    print(f"{kind} G={groups} {grid_name}: T {mesh['triangle_offsets'].tolist()}, R {built[2]}, points {points.shape[1]} per group, hits {hits}, "
          f"points with ties {int((wants[math.inf]['ties'] > 1).sum())}")
    finite = points.shape[0] * (points.shape[1] - len(range(*sets["not_finite"].indices(points.shape[1]))))
    assert hits[math.inf] == finite                                     # an infinite radius finds something for every finite point
    assert 0 < hits[radii(axes)[3]] < finite and hits[0.0] <= hits[radii(axes)[2]] <= hits[radii(axes)[3]]
    assert int((wants[math.inf]["ties"] > 1).sum()) > 0               # the tie rule decides some of these points


def test_outputs_in_every_optional_combination():
    mesh, axes, points, sets, wants = case("sphere", 3)
    dev = device_mesh(mesh)
    for grid_name in ("k2", "off_lattice"):
        grid = make_grid(grid_name, axes)
        built = run_build(dev, grid)
        for outputs in (("distance",), ("distance", "triangle"), ("distance", "triangle", "point"), ("distance", "triangle", "barycentric"), OUTPUTS):
            for radius in (math.inf, radii(axes)[3]):
                got = run_closest(dev, grid, built, points, radius, outputs)
                assert set(got) == set(outputs)
                assert_closest_equal(got, wants[radius], (grid_name, outputs, radius), sets, skip=sets["beyond"])


@pytest.mark.parametrize("count", [1, 77])
def test_one_point_and_a_count_that_is_no_multiple_of_64(count):
    mesh, axes, points, sets, _ = case("torus", 3)
    inside = np.concatenate([np.arange(sl.start, sl.stop) for name, sl in sets.items() if name != "beyond"])
    pick = inside[np.linspace(0, len(inside) - 1, count).astype(np.int64)]
    points = points[:, pick]
    grid = make_grid("k2", axes)
    dev = device_mesh(mesh)
    for radius in (math.inf, radii(axes)[3]):
        assert_closest_equal(run_closest(dev, grid, run_build(dev, grid), points, radius), cr.closest(mesh, points, radius), (count, radius))


def test_five_groups_with_empty_meshes_between_and_an_empty_mesh():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    parts = []
    for g, kind in enumerate(["torus", "all_outside", "noise", "all_inside", "sphere"]):
        field, level = make_field(kind, shape, axes, seed=50 + g)
        parts.append(sr.extract_surface(field[None], axes, level))
    mesh = pack(parts)
    to = mesh["triangle_offsets"].tolist()
    assert to[1] == to[2] and to[3] == to[4] and to[0] < to[1] < to[3] < to[5]
    points, sets = make_batch(mesh, axes, 4)
    tables = cr.pair_table(mesh, points)
    dev = device_mesh(mesh)
    for radius in (math.inf, radii(axes)[3]):
        want = cr.closest(mesh, points, radius, tables)
        for grid_name in ("k2", "off_lattice"):
            grid = make_grid(grid_name, axes)
            got = run_closest(dev, grid, run_build(dev, grid), points, radius)
            assert_closest_equal(got, want, ("five groups", grid_name, radius), sets, skip=sets["beyond"])
        assert int((want["triangle"][1] >= 0).sum()) == 0 and int((want["triangle"][3] >= 0).sum()) == 0 and int((want["triangle"][0] >= 0).sum()) > 0
    # an entirely empty mesh and an infinite radius: no reference outside the loose list, the call walks nothing and returns misses
    empty = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32), "vertex_offsets": np.zeros(3, np.int32),
             "triangle_offsets": np.zeros(3, np.int32)}
    dev = device_mesh(empty)
    grid = make_grid("k2", axes)
    built = run_build(dev, grid)
    assert built[2] == 0
    got = run_closest(dev, grid, built, points[:2], math.inf)
    assert bool((got["distance"] == math.inf).all()) and bool((got["triangle"] == -1).all())
    assert bool((got["point"] == 0).all()) and bool((got["barycentric"] == 0).all())


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
        tables = cr.pair_table(changed, points)
        dev = device_mesh(changed)
        for radius in (math.inf, radii(axes)[3]):
            want = cr.closest(changed, points, radius, tables)
            for grid_name in ("k2", "off_lattice"):
                grid = make_grid(grid_name, axes)
                got = run_closest(dev, grid, run_build(dev, grid), points, radius)
                assert_closest_equal(got, want, (name, grid_name, radius), sets, skip=sets["beyond"])
            assert int((want["triangle"] >= 0).sum()) > 0


def test_a_stale_grid_costs_correctness_never_memory_safety():
    """The lists of another mesh (and of a hostile one) with this mesh's arrays: guard rows intact, the call returns, and what it
    reports is an accepted candidate of the rule."""
    mesh, axes, points, sets, _ = case("sphere", 3)
    other, _, _ = mesh_case("noise", 3)
    grid = make_grid("k2", axes)
    for source in (other, hostile(other)):
        built = run_build(device_mesh(source), grid)
        dev = device_mesh(mesh)
        for radius in (math.inf, radii(axes)[3]):
            got = run_closest(dev, grid, built, points, radius)
            assert_candidates(mesh, points, got, radius)
    poisoned_lists = (poisoned((lists_of(device_mesh(mesh), grid) + 1,), torch.int32), poisoned((64,), torch.int32), 64)
    got = run_closest(device_mesh(mesh), grid, poisoned_lists, points, math.inf)
    assert_candidates(mesh, points, got, math.inf)


def test_the_same_call_twice_and_a_grid_built_twice_give_equal_bits():
    """The lists fill in the order of arrival, which differs from build to build; the query's results must not."""
    mesh, axes, points, sets, wants = case("noise", 1)
    grid = make_grid("k4", axes)
    dev = device_mesh(mesh)
    first, second = run_build(dev, grid), run_build(dev, grid)
    a, b, c = run_closest(dev, grid, first, points, math.inf), run_closest(dev, grid, first, points, math.inf), run_closest(dev, grid, second, points, math.inf)
    for key in a:
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
        assert torch.equal(a[key].view(torch.int32), c[key].view(torch.int32)), key


# ---------------------------------------------------------------------------------------------------------------------
# 2. a recorded call
def test_recorded_query_is_one_kernel_and_replays_on_other_points():
    mesh, axes, points, sets, wants = case("sphere", 3)
    other, _ = make_batch(mesh, axes, points_per_set(mesh), seed=1)
    grid = make_grid("k2", axes)
    dev = device_mesh(mesh)
    cell_offsets, references, R = run_build(dev, grid)
    G, N = points.shape[:2]
    p = torch.zeros((G, N, 3), device="cuda")
    out = {"distance": poisoned((G * N + GUARD,), torch.float32), "triangle": poisoned((G * N + GUARD,), torch.int32),
           "point": poisoned((G * N + GUARD, 3), torch.float32), "barycentric": poisoned((G * N + GUARD, 2), torch.float32)}
    s = surface.closest_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                               cell_offsets, references=references[:R], points=p, max_distance=math.inf, **out)
    lib = _lib.load()
    call = lambda: _lib.check(lib.pr_closest_query(C.byref(s), torch.cuda.current_stream().cuda_stream), "pr_closest_query")
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
    for batch, want in ((other, cr.closest(mesh, other, math.inf)), (points, wants[math.inf]), (other, None)):
        p.copy_(torch.from_numpy(batch))
        for t in out.values():
            t.view(torch.int32).fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        got = {key: t[:G * N].reshape((G, N) + tuple(t.shape[1:])) for key, t in out.items()}
        if want is not None:
            assert_closest_equal(got, want, "replay", sets, skip=sets["beyond"])
        assert all(bool(is_poison(t[G * N:]).all()) for t in out.values())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the python layer
def found_dict(found):
    out = {"distance": found.distance, "triangle": found.triangle}
    for key in ("point", "barycentric"):
        if getattr(found, key) is not None:
            out[key] = getattr(found, key)
    return out


def test_ray_grid_closest_nearest_and_distance_to():
    mesh, axes, points, sets, wants = case("sphere", 3)
    meshes = to_meshes(mesh)
    grid = surface.RayGrid.build(meshes, *surface.bounding_grid(meshes, (12, 16, 20)))
    to_cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    inside = np.concatenate([np.arange(sl.start, sl.stop) for name, sl in sets.items() if name != "beyond"])
    radius = radii(axes)[3]
    p = points[:, inside]
    found = grid.closest(to_cuda(p), max_distance=radius, point=True, barycentric=True, nearest=True)
    want = {key: value[:, inside] for key, value in wants[radius].items()}
    assert_closest_equal(found_dict(found), want, "RayGrid.closest")
    least, group = torch.min(found.distance, dim=0)
    assert torch.equal(found.nearest_distance, least) and found.group.dtype == torch.int64
    assert torch.equal(found.group, torch.where(torch.isinf(least), torch.full_like(group, -1), group))
    assert int((found.group >= 0).sum()) > 0 and int((found.group < 0).sum()) > 0
    bare = grid.closest(to_cuda(p), max_distance=radius)
    assert bare.point is None and bare.barycentric is None and bare.nearest_distance is None and bare.group is None
    assert torch.equal(bare.distance, found.distance) and torch.equal(bare.triangle, found.triangle)
    # (N, 3) points are used for every group
    shared = grid.closest(to_cuda(p[0]), max_distance=math.inf, point=True, barycentric=True)
    assert_closest_equal(found_dict(shared), cr.closest(mesh, np.broadcast_to(p[:1], p.shape).copy(), math.inf), "shared points")
    assert list(grid.closest(to_cuda(p[:, :0]), max_distance=1.0).distance.shape) == [3, 0]
    # Mesh.distance_to: the vertices of one mesh against another, given as a mesh or as a grid of one group
    one = {"vertices": mesh["vertices"][mesh["vertex_offsets"][1]:mesh["vertex_offsets"][2]],
           "triangles": mesh["triangles"][mesh["triangle_offsets"][1]:mesh["triangle_offsets"][2]]}
    one = pack([one])
    want = cr.closest(one, meshes[0].vertices.cpu().numpy()[None], math.inf)["distance"][0]
    deviation = meshes[0].distance_to(meshes[1], max_distance=math.inf, cells=8)
    assert deviation.shape == (meshes[0].vertices.size(0),) and np.array_equal(deviation.cpu().numpy().view(np.int32), want.view(np.int32))
    again = meshes[0].distance_to(meshes[1].ray_grid(*make_grid("k2", axes)), max_distance=math.inf)
    assert torch.equal(again, deviation) and float(deviation.max()) > 0
    assert float(meshes[0].distance_to(meshes[0], max_distance=1.0, cells=8).max()) == 0.0      # every vertex lies on its own mesh
    for bad in (lambda: grid.closest(to_cuda(p[:2]), max_distance=1.0), lambda: grid.closest(to_cuda(p[..., :2]), max_distance=1.0),
                lambda: grid.closest(to_cuda(p), max_distance=math.nan), lambda: grid.closest(to_cuda(p), max_distance=-1.0),
                lambda: meshes[0].distance_to(grid, max_distance=1.0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        grid.closest(to_cuda(p))                                          # max_distance has no default


# ---------------------------------------------------------------------------------------------------------------------
# 4. the composer
@pytest.mark.parametrize("simplify", [0, 2])
def test_points_against_the_composers_own_mesh(simplify):
    """``extract_mesh`` of the small tennis ``player_1`` network: the point sets against the mesh's own grids (simplify=0), and the
    vertices of the simplified mesh against the grid of the full mesh - the deviation measure (simplify=2)."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        meshes = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level)
        simplified = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, simplify=2) if simplify else None
    mesh = pack([{"vertices": m.vertices.cpu().numpy(), "triangles": m.triangles.cpu().numpy()} for m in meshes])
    axes = [centres[:, 0, 0, 0].cpu().numpy(), centres[0, :, 0, 1].cpu().numpy(), centres[0, 0, :, 2].cpu().numpy()]
    assert mesh["triangle_offsets"][1] > 0 and mesh["triangle_offsets"][2] > mesh["triangle_offsets"][1]
    to_cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if simplify == 0:
        grids = (surface.lattice_cluster_grid(axes, 2), surface.bounding_grid(meshes, 16))
        step = min(min(g[1]) for g in grids)
        points, sets = cr.point_batch(mesh, axes, 4, [grids[0], make_grid("off_lattice", axes)], step)
        skip = sets["beyond"]
    else:
        grids = (surface.bounding_grid(meshes, 16),)
        count = min(m.vertices.size(0) for m in simplified)
        pick = lambda m: m.vertices[torch.linspace(0, m.vertices.size(0) - 1, min(count, 64)).long()]
        points, sets, skip = torch.stack([pick(m) for m in simplified]).cpu().numpy(), None, None
    want = cr.closest(mesh, points, math.inf)
    for grid in grids:
        found = surface.RayGrid.build(meshes, *grid).closest(to_cuda(points), max_distance=math.inf, point=True, barycentric=True)
        assert_closest_equal(found_dict(found), want, ("composer", simplify), sets, skip=skip)
    print(f"simplify={simplify}: T {mesh['triangle_offsets'].tolist()}, points {points.shape[1]} per group, largest distance "
          f"{float(np.max(np.where(np.isfinite(want['distance']), want['distance'], 0))):.4g}")
    assert int((want["triangle"] >= 0).sum()) > 0

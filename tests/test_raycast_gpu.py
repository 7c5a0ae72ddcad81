"""Ray queries on the GPU (python -m pytest tests -m gpu): ``pr_raycast_build`` / ``pr_raycast_query`` against the exhaustive numpy
search (tests/raycast_reference.py) bit for bit - ``t`` as bits, ``triangle``, ``barycentric`` - for every ray of every set, on the
meshes of tests/surface_reference.py in one and three groups, on five grids; the lists of the build against the header's
classification; poisoned memory with guard rows, counting builds, short capacities, repeated and recorded calls; the Python layer and
``ObjectComposer.extract_mesh`` on the small tennis networks.  The reference does not depend on the grid, so one search per (mesh, ray
batch, window) serves all grids."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from playableenvironments_amd import Mesh, _lib, frame_graph, surface
from tests import raycast_reference as rr
from tests import simplify_reference as sp
from tests import surface_reference as sr
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, make_field, poisoned, tennis

pytestmark = pytest.mark.gpu

F = np.float32
OFF_LATTICE = ([-0.7, -0.71, -0.69], [0.11, 0.13, 0.17], [13, 11, 9])
GRIDS = ["one_cell", "k2", "k4", "off_lattice", "column"]
MESHES = ["sphere", "torus", "plane", "noise", "equal_to_level", "simplified"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes, grids, rays (numpy only: nothing here needs a GPU)
def pack(parts):
    """Packed dict of single-group mesh dicts."""
    return {"vertices": np.concatenate([p["vertices"] for p in parts]).reshape(-1, 3).astype(F),
            "triangles": np.concatenate([p["triangles"] for p in parts]).reshape(-1, 3).astype(np.int32),
            "vertex_offsets": np.concatenate([[0], np.cumsum([len(p["vertices"]) for p in parts])]).astype(np.int32),
            "triangle_offsets": np.concatenate([[0], np.cumsum([len(p["triangles"]) for p in parts])]).astype(np.int32)}


_PARTS = {}


def part(kind, seed=0):
    """(single-group mesh dict, lattice axes) of one of the shared fields; computed once."""
    if (kind, seed) not in _PARTS:
        if kind in ("sphere", "torus"):
            field, axes = (sr.sphere_field if kind == "sphere" else sr.torus_field)(17)
            level = 0.0
        elif kind == "plane":
            field, axes = sr.plane_field()                       # non-uniform axes
            level = 1.4
        elif kind == "simplified":
            field, axes = sr.sphere_field(33)
            fine = sr.extract_surface(field[None], axes, 0.0)
            _PARTS[(kind, seed)] = (sp.simplify_mesh(fine, *sp.lattice_grid(axes, 2)), axes)
            return _PARTS[(kind, seed)]
        else:
            shape = (17, 17, 17) if kind == "noise17" else (9, 17, 33)
            axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
            field, level = make_field("noise" if kind == "noise17" else kind, shape, axes, seed=3 + seed)
        _PARTS[(kind, seed)] = (sr.extract_surface(field[None], axes, level), axes)
    return _PARTS[(kind, seed)]


def mesh_case(kind, groups):
    """(packed mesh, axes of the first group's lattice, rays per set)."""
    first, axes = part(kind)
    if groups == 1:
        parts = [first]
    elif kind == "plane":
        parts = [first, part("plane")[0], first]
    else:
        parts = [first, part("torus" if kind == "sphere" else "sphere")[0], part(kind, seed=1)[0]]
    mesh = pack(parts)
    return mesh, axes, 192 if mesh["triangle_offsets"][-1] < 12000 else 48


def make_grid(name, axes):
    first, extent = [float(a[0]) for a in axes], [float(a[-1]) - float(a[0]) for a in axes]
    if name[0] == "k":
        return sp.lattice_grid(axes, int(name[1:]))
    if name == "one_cell":
        return first, extent, [1, 1, 1]
    if name == "column":
        return first, [extent[0], extent[1], extent[2] / 64], [1, 1, 64]
    return OFF_LATTICE


def unit(rng, n):
    x = rng.normal(size=(n, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def ray_batch(mesh, axes, n, seed=0):
    """``(origins, directions (G, N, 3), sets)``: every ray set of the issue, ``n`` rays each, concatenated; ``sets`` names the
    slices.  The sets that lie in cell faces and pass through cell corners use the k = 2 lattice grid and the off-lattice grid."""
    rng = np.random.default_rng(100 + seed)
    centre = np.array([(float(a[0]) + float(a[-1])) / 2 for a in axes])
    half = np.array([(float(a[-1]) - float(a[0])) / 2 for a in axes])
    far = 3 * half.max()
    G = len(mesh["vertex_offsets"]) - 1
    all_o, all_d, sets = [], [], {}
    for g, (vertices, triangles) in enumerate(rr.group_slices(mesh)):
        o_parts, d_parts, at = [], [], 0

        def add(name, o, d):
            nonlocal at
            o_parts.append(np.asarray(o, dtype=F))
            d_parts.append(np.asarray(d, dtype=F))
            sets[name] = slice(at, at + len(o))
            at += len(o)

        outside = (centre + far * unit(rng, n)).astype(F)
        add("outside", outside, (centre + 0.5 * half * rr.ball_points(rng, n, 1.0)).astype(F) - outside)
        add("inside", (centre + 0.45 * half * rr.ball_points(rng, n, 1.0)).astype(F), (unit(rng, n) * rng.uniform(0.1, 4, (n, 1))).astype(F))
        good = triangles[np.all((triangles >= 0) & (triangles < max(len(vertices), 1)), axis=1)] if len(vertices) else triangles[:0]
        if len(good):
            tri = good[rng.integers(0, len(good), n)]
            corner = np.nan_to_num(vertices[tri[:, 0]], nan=0.0, posinf=0.0, neginf=0.0)
            middle = np.nan_to_num((vertices[tri[:, 1]] + vertices[tri[:, 2]]) * F(0.5), nan=0.0, posinf=0.0, neginf=0.0)
        else:
            corner = middle = np.zeros((n, 3), dtype=F)
        o = (centre + far * unit(rng, n)).astype(F)
        add("vertices", o, corner - o)
        add("midpoints", o, middle - o)
        # axis-parallel: two zero components, then one
        axis = rng.integers(0, 3, n)
        o = (centre + half * rng.uniform(-0.9, 0.9, (n, 3))).astype(F)
        o[np.arange(n), axis] = F(centre[axis] - far)
        d = np.zeros((n, 3), dtype=F)
        d[np.arange(n), axis] = rng.uniform(0.5, 2, n)
        add("two_zeros", o, d)
        d = d.copy()
        d[np.arange(n), (axis + 1) % 3] = rng.uniform(-0.3, 0.3, n)
        add("one_zero", o, d)
        # in cell faces and through cell corners of two grids
        for tag, (origin, cell, cells) in (("k2", make_grid("k2", axes)), ("off", OFF_LATTICE)):
            origin, cell = np.asarray(origin, dtype=F), np.asarray(cell, dtype=F)
            axis = rng.integers(0, 3, n)
            plane = np.stack([rng.integers(0, c + 1, n) for c in cells], axis=1)
            on_planes = origin + plane.astype(F) * cell                             # fp32: the planes as the library sees them
            o = (centre + half * rng.uniform(-0.9, 0.9, (n, 3))).astype(F)
            run = (axis + 1) % 3
            o[np.arange(n), axis] = on_planes[np.arange(n), axis]
            o[np.arange(n), run] = F(centre[run] - far)
            d = np.zeros((n, 3), dtype=F)
            d[np.arange(n), run] = 1
            d[np.arange(n), (axis + 2) % 3] = rng.uniform(-0.2, 0.2, n)
            add("faces_" + tag, o, d)
            o = (centre + far * unit(rng, n)).astype(F)
            add("corners_" + tag, o, on_planes - o)
        o = (centre + far * unit(rng, n)).astype(F)
        add("missing", o, (o - centre.astype(F)) * rng.uniform(0.1, 2, (n, 1)).astype(F) + unit(rng, n).astype(F))
        add("zero_direction", (centre + half * rng.uniform(-1, 1, (n, 3))).astype(F), np.zeros((n, 3), dtype=F))
        o = (centre + far * unit(rng, n)).astype(F)
        d = (centre - o).astype(F)
        bad = rng.integers(0, 6, n)
        value = np.array([np.nan, np.inf, -np.inf], dtype=F)[rng.integers(0, 3, n)]
        o, d = o.copy(), d.copy()
        o[np.arange(n)[bad < 3], bad[bad < 3]] = value[bad < 3]
        d[np.arange(n)[bad >= 3], bad[bad >= 3] - 3] = value[bad >= 3]
        add("not_finite", o, d)
        o = (centre + 0.5 * far * unit(rng, n)).astype(F)
        add("behind", o, o - (centre + 0.3 * half * rr.ball_points(rng, n, 1.0)).astype(F))      # the mesh lies at negative t
        all_o.append(np.concatenate(o_parts))
        all_d.append(np.concatenate(d_parts))
    assert len(all_o) == G
    return np.stack(all_o), np.stack(all_d), sets


_BATCH, _WANT = {}, {}


def batch(key, mesh, axes, n):
    if key not in _BATCH:
        _BATCH[key] = ray_batch(mesh, axes, n)
    return _BATCH[key]


def reference(key, mesh, o, d, t_min=0.0, t_max=np.inf, cull_back=False):
    key = (key, float(t_min), float(t_max), cull_back, o.shape)
    if key not in _WANT:
        _WANT[key] = rr.cast(mesh, o, d, t_min, t_max, cull_back)
    return _WANT[key]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def device_mesh(mesh):
    """The packed input as device tensors (at least one row each: an empty tensor has no address)."""
    pad = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros((1, 3), dtype=a.dtype))).to(dtype).cuda()
    return {"vertices": pad(mesh["vertices"], torch.float32), "triangles": pad(mesh["triangles"], torch.int32),
            "vertex_offsets": torch.from_numpy(np.asarray(mesh["vertex_offsets"], dtype=np.int32)).cuda(),
            "triangle_offsets": torch.from_numpy(np.asarray(mesh["triangle_offsets"], dtype=np.int32)).cuda(),
            "V": int(mesh.get("V", len(mesh["vertices"]))), "T": int(mesh.get("T", len(mesh["triangles"])))}


def lists_of(dev, grid):
    return (dev["vertex_offsets"].numel() - 1) * (grid[2][0] * grid[2][1] * grid[2][2] + 1)


def build_call(dev, grid, cell_offsets, references=None, capacity=None):
    s = surface.raycast_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                               cell_offsets, references=references)
    if capacity is not None:
        s.max_references = capacity
    size = C.c_size_t()
    _lib.check(_lib.load().pr_raycast_workspace_size(C.byref(s), C.byref(size)), "pr_raycast_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")          # (64 guard words)
    return s, workspace, size.value


def launch_build(s, workspace, size):
    _lib.check(_lib.load().pr_raycast_build(C.byref(s), workspace.data_ptr(), size, torch.cuda.current_stream().cuda_stream), "pr_raycast_build")


def run_build(dev, grid, capacity=None, count_only=False):
    """A counting call, the read-back of R and (unless ``count_only``) an emitting call with ``capacity`` (default: R) rows, all on
    poisoned memory with guard rows.  Returns (cell_offsets, references, R)."""
    lists = lists_of(dev, grid)
    cell_offsets = poisoned((lists + 1 + GUARD,), torch.int32)
    s, workspace, size = build_call(dev, grid, cell_offsets)
    launch_build(s, workspace, size)
    torch.cuda.synchronize()
    R = int(cell_offsets[lists])
    assert bool(is_poison(cell_offsets[lists + 1:]).all()) and bool(is_poison(workspace[size // 4:]).all())
    if count_only:
        return cell_offsets, None, R
    capacity = R if capacity is None else capacity
    references = poisoned((max(capacity, 0) + GUARD,), torch.int32)
    counted = cell_offsets.clone()
    s, workspace, size = build_call(dev, grid, cell_offsets, references, capacity)
    launch_build(s, workspace, size)
    torch.cuda.synchronize()
    assert torch.equal(cell_offsets, counted)                              # the emitting call reports the same offsets and R
    assert bool(is_poison(references[capacity:]).all()) and bool(is_poison(workspace[size // 4:]).all())
    return cell_offsets, references, R


def query_call(dev, grid, cell_offsets, references, R, origins, directions, out, **kw):
    return surface.raycast_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], *grid,
                                  cell_offsets, references=references[:R] if R else None, origins=origins, directions=directions,
                                  t=out["t"], triangle=out.get("triangle"), barycentric=out.get("barycentric"), **kw)


def run_query(dev, grid, built, o, d, triangle=True, barycentric=True, **kw):
    cell_offsets, references, R = built
    G, N = o.shape[:2]
    origins, directions = torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    out = {"t": poisoned((G * N + GUARD,), torch.float32)}
    if triangle:
        out["triangle"] = poisoned((G * N + GUARD,), torch.int32)
    if barycentric:
        out["barycentric"] = poisoned((G * N + GUARD, 2), torch.float32)
    s = query_call(dev, grid, cell_offsets, references, R, origins, directions, out, **kw)
    _lib.check(_lib.load().pr_raycast_query(C.byref(s), torch.cuda.current_stream().cuda_stream), "pr_raycast_query")
    torch.cuda.synchronize()
    for key, t in out.items():
        assert bool(is_poison(t[G * N:]).all()), key
    return {key: t[:G * N].reshape((G, N) + tuple(t.shape[1:])) for key, t in out.items()}


def assert_hits_equal(got, want, what, sets=None):
    """Every ray: ``t`` as bits, ``triangle``, ``barycentric`` as bits."""
    t = got["t"].cpu().numpy()
    same = t.view(np.int32) == want["t"].view(np.int32)
    if "triangle" in got:
        same &= got["triangle"].cpu().numpy() == want["triangle"]
    if "barycentric" in got:
        same &= np.all(got["barycentric"].cpu().numpy().view(np.int32) == want["barycentric"].view(np.int32), axis=-1)
    if not same.all():
        g, r = np.argwhere(~same)[0]
        name = [k for k, sl in (sets or {}).items() if sl.start <= r < sl.stop]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} rays differ; first: group {g} ray {r} {name}: got t {t[g, r]!r} "
                             f"triangle {int(got['triangle'][g, r]) if 'triangle' in got else None}, want t {want['t'][g, r]!r} "
                             f"triangle {int(want['triangle'][g, r])}")


def assert_lists_equal(built, mesh, grid, what):
    """``cell_offsets`` against the numpy count of the padded boxes, every list as a sorted set."""
    cell_offsets, references, R = built
    want = rr.grid_lists(mesh, *grid)
    sizes = np.array([len(l) for group in want for l in group], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    got = cell_offsets[:len(offsets)].cpu().numpy()
    assert np.array_equal(got, offsets), (what, int((got != offsets).sum()))
    assert R == offsets[-1], (what, R, offsets[-1])
    if references is None:
        return
    refs = references[:R].cpu().numpy()
    flat = [l for group in want for l in group]
    for i, l in enumerate(flat):
        assert np.array_equal(np.sort(refs[offsets[i]:offsets[i + 1]]), l), (what, i)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit identity through the C ABI
@pytest.mark.parametrize("grid_name", GRIDS)
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", MESHES)
def test_hits_equal_the_exhaustive_search(kind, groups, grid_name):
    mesh, axes, n = mesh_case(kind, groups)
    grid = make_grid(grid_name, axes)
    o, d, sets = batch((kind, groups), mesh, axes, n)
    want = reference((kind, groups), mesh, o, d)
    dev = device_mesh(mesh)
    built = run_build(dev, grid)
    if mesh["triangle_offsets"][-1] < 12000:
        assert_lists_equal(built, mesh, grid, (kind, groups, grid_name))
    got = run_query(dev, grid, built, o, d)
    hits = int((want["triangle"] >= 0).sum())
    loose = int(sum(int(built[0][(g + 1) * (lists_of(dev, grid) // groups)] - built[0][(g + 1) * (lists_of(dev, grid) // groups) - 1])
                    for g in range(groups)))
    print(f"{kind} G={groups} {grid_name}: T {mesh['triangle_offsets'].tolist()}, R {built[2]}, loose {loose}, rays {o.shape[1]} per group, "
          f"hits {hits}, rays with ties {int((want['ties'] > 1).sum())}")
    assert_hits_equal(got, want, (kind, groups, grid_name), sets)
    assert hits > 0 and int((want["triangle"][:, sets["zero_direction"]] >= 0).sum()) == 0
    assert int((want["triangle"][:, sets["not_finite"]] >= 0).sum()) == 0
    if kind in ("sphere", "torus"):
        assert int((want["ties"] > 1).sum()) > 0                           # the tie rule decides some of these rays


@pytest.mark.parametrize("grid_name", ["k2", "off_lattice", "column"])
def test_windows_culling_and_negative_t(grid_name):
    """Windows that select the second hit, hits behind the origin, back-face culling, and outputs left out."""
    mesh, axes, _ = mesh_case("sphere", 3)
    grid = make_grid(grid_name, axes)
    o, d, sets = batch(("sphere", 3, "windows"), mesh, axes, 64)          # (eight searches: a third of the usual rays per set)
    dev = device_mesh(mesh)
    built = run_build(dev, grid)
    first = reference(("sphere", 3), mesh, o, d)
    for t_min, t_max, cull in ((0.0, np.inf, True), (-np.inf, np.inf, False), (-100.0, 0.0, False), (-np.inf, np.inf, True),
                               (0.9, 1.5, False), (1.0, 1.0, False), (2.0, 0.5, False), (np.inf, np.inf, False)):
        want = reference(("sphere", 3), mesh, o, d, t_min, t_max, cull)
        got = run_query(dev, grid, built, o, d, t_min=t_min, t_max=t_max, cull_back=cull)
        assert_hits_equal(got, want, (grid_name, t_min, t_max, cull), sets)
    second = reference(("sphere", 3), mesh, o, d, 0.9, 1.5)
    later = (second["triangle"] >= 0) & (first["triangle"] >= 0) & (second["t"] > first["t"])
    assert int(later[:, sets["outside"]].sum()) > 0                        # (the directions span the sphere: its far side lies near t = 1.2)
    behind = reference(("sphere", 3), mesh, o, d, -100.0, 0.0)
    assert int((behind["t"][:, sets["behind"]] < 0).sum()) > 0
    want = reference(("sphere", 3), mesh, o, d)
    assert_hits_equal(run_query(dev, grid, built, o, d, triangle=False, barycentric=False), want, "t alone")
    assert_hits_equal(run_query(dev, grid, built, o, d, barycentric=False), want, "t and triangle")


@pytest.mark.parametrize("rays", [1, 77])
def test_one_ray_and_a_count_that_is_no_multiple_of_64(rays):
    mesh, axes, n = mesh_case("torus", 3)
    o, d, sets = batch(("torus", 3), mesh, axes, n)
    pick = np.linspace(0, o.shape[1] - 1, rays).astype(np.int64)
    o, d = o[:, pick], d[:, pick]
    grid = make_grid("k2", axes)
    dev = device_mesh(mesh)
    assert_hits_equal(run_query(dev, grid, run_build(dev, grid), o, d), rr.cast(mesh, o, d), rays)


def test_five_groups_with_empty_meshes_between():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    parts = []
    for g, kind in enumerate(["torus", "all_outside", "noise", "all_inside", "sphere"]):
        field, level = make_field(kind, shape, axes, seed=50 + g)
        parts.append(sr.extract_surface(field[None], axes, level))
    mesh = pack(parts)
    to = mesh["triangle_offsets"].tolist()
    assert to[1] == to[2] and to[3] == to[4] and to[0] < to[1] < to[3] < to[5]
    o, d, sets = ray_batch(mesh, axes, 32)
    want = rr.cast(mesh, o, d)
    dev = device_mesh(mesh)
    for grid_name in ("k2", "off_lattice"):
        grid = make_grid(grid_name, axes)
        assert_hits_equal(run_query(dev, grid, run_build(dev, grid), o, d), want, ("five groups", grid_name), sets)
    assert int((want["triangle"][1] >= 0).sum()) == 0 and int((want["triangle"][3] >= 0).sum()) == 0 and int((want["triangle"][0] >= 0).sum()) > 0
    empty = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32), "vertex_offsets": np.zeros(3, np.int32),
             "triangle_offsets": np.zeros(3, np.int32)}
    dev = device_mesh(empty)
    built = run_build(dev, grid)
    assert built[2] == 0
    got = run_query(dev, grid, built, o[:2], d[:2])
    assert bool((got["t"] == math.inf).all()) and bool((got["triangle"] == -1).all()) and bool((got["barycentric"] == 0).all())


def hostile(mesh, seed=1):
    """A copy with NaN and +-inf coordinates, triangle indices -1, V_g and 2^31 - 1, and offsets that decrease and leave the arrays."""
    rng = np.random.default_rng(seed)
    out = {k: v.copy() for k, v in mesh.items()}
    pick = rng.uniform(0, 1, out["vertices"].shape)
    out["vertices"][pick < 0.01] = np.nan
    out["vertices"][(pick >= 0.01) & (pick < 0.015)] = np.inf
    out["vertices"][(pick >= 0.015) & (pick < 0.02)] = -np.inf
    to, vo = out["triangle_offsets"], out["vertex_offsets"]
    for g in range(len(to) - 1):
        rows = np.arange(to[g], to[g + 1])
        pick = rng.uniform(0, 1, len(rows))
        out["triangles"][rows[pick < 0.03], 1] = -1
        out["triangles"][rows[(pick >= 0.03) & (pick < 0.06)], 2] = vo[g + 1] - vo[g]
        out["triangles"][rows[(pick >= 0.06) & (pick < 0.07)], 0] = 2 ** 31 - 1
    return out


def test_hostile_meshes_and_offsets():
    mesh, axes, n = mesh_case("sphere", 3)
    o, d, sets = batch(("sphere", 3), mesh, axes, n)
    bad = hostile(mesh)
    V, T = len(mesh["vertices"]), len(mesh["triangles"])
    cases = [("values", bad)]
    for name, vo, to in (("decreasing", [0, mesh["vertex_offsets"][2], mesh["vertex_offsets"][1], V], [0, mesh["triangle_offsets"][2], mesh["triangle_offsets"][1], T]),
                         ("leaving", [-5, mesh["vertex_offsets"][1], V + 1000, 2 ** 31 - 1], [-2 ** 31, mesh["triangle_offsets"][1], T + 7, T + 9])):
        case = dict(bad)
        case["vertex_offsets"], case["triangle_offsets"] = np.array(vo, dtype=np.int32), np.array(to, dtype=np.int32)
        cases.append((name, case))
    for name, case in cases:
        want = rr.cast(case, o, d, -np.inf, np.inf)
        dev = device_mesh(case)
        for grid_name in ("k2", "off_lattice"):
            grid = make_grid(grid_name, axes)
            built = run_build(dev, grid)
            assert_lists_equal(built, case, grid, (name, grid_name))
            assert_hits_equal(run_query(dev, grid, built, o, d, t_min=-math.inf), want, (name, grid_name), sets)
        assert int((want["triangle"] >= 0).sum()) > 0


def test_counting_builds_and_short_capacities_report_r():
    mesh, axes, _ = mesh_case("torus", 3)
    grid = make_grid("k2", axes)
    dev = device_mesh(mesh)
    full = run_build(dev, grid)
    R = full[2]
    assert R > 1000
    counted = run_build(dev, grid, count_only=True)
    assert counted[2] == R and torch.equal(counted[0], full[0])
    lists = lists_of(dev, grid)
    offsets = full[0][:lists + 1].cpu().numpy()
    for capacity in (R // 2, 0, 1):
        cell_offsets, references, reported = run_build(dev, grid, capacity=capacity)
        assert reported == R and torch.equal(cell_offsets, full[0])
        refs, all_refs = references[:capacity].cpu().numpy(), full[1][:R].cpu().numpy()
        # a prefix: every written slot holds a triangle of the list the slot belongs to, and the rest of the rows was never touched
        owner = np.searchsorted(offsets, np.arange(capacity), side="right") - 1
        for i in np.unique(owner):
            mine = refs[np.arange(capacity)[owner == i]]
            assert np.isin(mine, all_refs[offsets[i]:offsets[i + 1]]).all() and len(np.unique(mine)) == len(mine)


def test_the_same_calls_twice_give_equal_bits():
    """The lists fill in the order of arrival, which differs from run to run; the offsets and the query's results must not."""
    mesh, axes, n = mesh_case("noise", 1)
    grid = make_grid("k4", axes)
    o, d, _ = batch(("noise", 1), mesh, axes, n)
    dev = device_mesh(mesh)
    first, second = run_build(dev, grid), run_build(dev, grid)
    assert torch.equal(first[0], second[0]) and first[2] == second[2]
    a, b = run_query(dev, grid, first, o, d), run_query(dev, grid, second, o, d)
    for key in a:
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key


# ---------------------------------------------------------------------------------------------------------------------
# 2. recorded calls
def test_recorded_build_and_query_hold_kernels_only_and_replay_on_other_data():
    first, axes, n = mesh_case("sphere", 3)
    second, _, _ = mesh_case("torus", 3)
    o1, d1, _ = batch(("sphere", 3), first, axes, n)
    o2, d2, _ = batch(("torus", 3), second, axes, n)
    V = max(len(first["vertices"]), len(second["vertices"]))
    T = max(len(first["triangles"]), len(second["triangles"]))
    grid = make_grid("k2", axes)
    room = {"vertices": np.zeros((V, 3), F), "triangles": np.zeros((T, 3), np.int32), "vertex_offsets": first["vertex_offsets"],
            "triangle_offsets": first["triangle_offsets"]}
    dev = device_mesh(room)
    lists = lists_of(dev, grid)
    capacity = 16 * T
    cell_offsets = poisoned((lists + 1 + GUARD,), torch.int32)
    references = poisoned((capacity + GUARD,), torch.int32)
    G, N = o1.shape[:2]
    origins, directions = torch.zeros((G, N, 3), device="cuda"), torch.zeros((G, N, 3), device="cuda")
    out = {"t": poisoned((G * N + GUARD,), torch.float32), "triangle": poisoned((G * N + GUARD,), torch.int32),
           "barycentric": poisoned((G * N + GUARD, 2), torch.float32)}
    b, workspace, size = build_call(dev, grid, cell_offsets, references, capacity)
    q = query_call(dev, grid, cell_offsets, references, capacity, origins, directions, out)
    lib = _lib.load()

    def record(call):
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
        return graph, census

    build_graph, build_census = record(lambda: launch_build(b, workspace, size))
    query_graph, query_census = record(lambda: _lib.check(lib.pr_raycast_query(C.byref(q), torch.cuda.current_stream().cuda_stream),
                                                          "pr_raycast_query"))
    print("recorded build:", build_census, "recorded query:", query_census)
    assert build_census == {"nodes": 7, "kernels": 7, "memsets": 0, "memcpys": 0}
    assert query_census == {"nodes": 1, "kernels": 1, "memsets": 0, "memcpys": 0}
    for mesh, o, d in ((second, o2, d2), (first, o1, d1), (second, o2, d2)):
        for key in ("vertices", "triangles"):
            dev[key].view(torch.int32).fill_(POISON)
            dev[key][:len(mesh[key])].copy_(torch.from_numpy(mesh[key]))
        dev["vertex_offsets"].copy_(torch.from_numpy(mesh["vertex_offsets"]))
        dev["triangle_offsets"].copy_(torch.from_numpy(mesh["triangle_offsets"]))
        origins.copy_(torch.from_numpy(o))
        directions.copy_(torch.from_numpy(d))
        for t in (cell_offsets, references, *out.values()):
            t.view(torch.int32).fill_(POISON)
        build_graph.replay()
        query_graph.replay()
        torch.cuda.synchronize()
        R = int(cell_offsets[lists])
        assert 0 < R <= capacity and bool(is_poison(references[R:]).all()) and bool(is_poison(workspace[size // 4:]).all())
        assert_lists_equal((cell_offsets, references, R), mesh, grid, "replay")
        got = {key: t[:G * N].reshape((G, N) + tuple(t.shape[1:])) for key, t in out.items()}
        assert_hits_equal(got, rr.cast(mesh, o, d), "replay")
        assert all(bool(is_poison(t[G * N:]).all()) for t in out.values())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the python layer
def to_meshes(mesh):
    vo, to = mesh["vertex_offsets"], mesh["triangle_offsets"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return [Mesh(cuda(mesh["vertices"][vo[g]:vo[g + 1]]), cuda(mesh["triangles"][to[g]:to[g + 1]])) for g in range(len(vo) - 1)]


def hits_dict(hits):
    out = {"t": hits.t, "triangle": hits.triangle}
    if hits.barycentric is not None:
        out["barycentric"] = hits.barycentric
    return out


def test_ray_grid_bounding_grid_and_nearest():
    mesh, axes, n = mesh_case("sphere", 3)
    o, d, sets = batch(("sphere", 3), mesh, axes, n)
    meshes = to_meshes(mesh)
    origin, cell, cells = surface.bounding_grid(meshes, (12, 16, 20))
    v = mesh["vertices"].astype(np.float64)
    for a in range(3):                                           # an eighth of a cell of room on every side
        assert cells[a] == (12, 16, 20)[a] and math.isclose(origin[a], v[:, a].min() - cell[a] / 8, rel_tol=1e-6, abs_tol=1e-7)
        assert math.isclose(origin[a] + cells[a] * cell[a], v[:, a].max() + cell[a] / 8, rel_tol=1e-6, abs_tol=1e-7)
    assert surface.bounding_grid(meshes, 8)[2] == [8, 8, 8]
    grid = surface.RayGrid.build(meshes, origin, cell, cells)
    assert grid.groups == 3 and grid.references.numel() == int(grid.cell_offsets[-1]) > 0
    C1 = cells[0] * cells[1] * cells[2] + 1                      # inside a bounding grid no well-shaped triangle is loose
    assert all(int(grid.cell_offsets[(g + 1) * C1] - grid.cell_offsets[(g + 1) * C1 - 1]) == 0 for g in range(3))
    want = reference(("sphere", 3), mesh, o, d)
    to_cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hits = grid.cast(to_cuda(o), to_cuda(d), barycentric=True, nearest=True)
    assert_hits_equal(hits_dict(hits), want, "RayGrid.cast", sets)
    least, group = torch.min(hits.t, dim=0)
    assert torch.equal(hits.nearest_t, least) and hits.group.dtype == torch.int64
    assert torch.equal(hits.group, torch.where(torch.isinf(least), torch.full_like(group, -1), group))
    assert int((hits.group >= 0).sum()) > 0 and int((hits.group < 0).sum()) > 0
    bare = grid.cast(to_cuda(o), to_cuda(d))
    assert bare.barycentric is None and bare.nearest_t is None and torch.equal(bare.t, hits.t) and torch.equal(bare.triangle, hits.triangle)
    culled = grid.cast(to_cuda(o), to_cuda(d), cull_back=True, t_min=0.25, t_max=9.0, barycentric=True)
    assert_hits_equal(hits_dict(culled), reference(("sphere", 3), mesh, o, d, 0.25, 9.0, True), "RayGrid.cast, culled", sets)
    # (N, 3) rays are used for every group
    shared = grid.cast(to_cuda(o[0]), to_cuda(d[0]), barycentric=True)
    same_o, same_d = np.broadcast_to(o[:1], o.shape).copy(), np.broadcast_to(d[:1], d.shape).copy()
    assert_hits_equal(hits_dict(shared), rr.cast(mesh, same_o, same_d), "shared rays")
    # one mesh
    single = meshes[1].ray_grid(*make_grid("k2", axes))
    one = {"vertices": meshes[1].vertices.cpu().numpy(), "triangles": meshes[1].triangles.cpu().numpy(),
           "vertex_offsets": np.array([0, meshes[1].vertices.size(0)], np.int32), "triangle_offsets": np.array([0, meshes[1].triangles.size(0)], np.int32)}
    assert_hits_equal(hits_dict(single.cast(to_cuda(o[1]), to_cuda(d[1]), barycentric=True)), rr.cast(one, o[1:2], d[1:2]), "Mesh.ray_grid")
    assert list(grid.cast(to_cuda(o[:, :0]), to_cuda(d[:, :0])).t.shape) == [3, 0]
    for bad in (lambda: grid.cast(to_cuda(o[:2]), to_cuda(d[:2])), lambda: grid.cast(to_cuda(o), to_cuda(d[:, :5])),
                lambda: grid.cast(to_cuda(o), to_cuda(d), t_min=math.nan), lambda: surface.RayGrid.build(meshes, [0, 0, 0], [1, 1, 1], [2048, 1, 1])):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the composer
@pytest.mark.parametrize("simplify", [0, 2])
def test_rays_against_the_composers_own_mesh(simplify):
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        meshes = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, simplify=simplify)
    mesh = pack([{"vertices": m.vertices.cpu().numpy(), "triangles": m.triangles.cpu().numpy()} for m in meshes])
    axes = [centres[:, 0, 0, 0].cpu().numpy(), centres[0, :, 0, 1].cpu().numpy(), centres[0, 0, :, 2].cpu().numpy()]
    assert mesh["triangle_offsets"][1] > 0 and mesh["triangle_offsets"][2] > mesh["triangle_offsets"][1]
    o, d, sets = ray_batch(mesh, axes, 48 if simplify == 0 else 128)
    want = rr.cast(mesh, o, d)
    to_cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for grid in (surface.lattice_cluster_grid(axes, 2), surface.bounding_grid(meshes, 16)):
        hits = surface.RayGrid.build(meshes, *grid).cast(to_cuda(o), to_cuda(d), barycentric=True)
        assert_hits_equal(hits_dict(hits), want, ("composer", simplify), sets)
    print(f"simplify={simplify}: T {mesh['triangle_offsets'].tolist()}, hits {int((want['triangle'] >= 0).sum())} of {want['t'].size}")
    assert int((want["triangle"] >= 0).sum()) > 0

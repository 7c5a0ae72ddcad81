"""Component labelling on the GPU (python -m pytest tests -m gpu): ``pr_label_components`` against the numpy restatement of its
contract (tests/components_reference.py) with ``torch.equal`` - labels, sizes, counts, and ``sigma_out`` as int32 bit patterns so that
NaNs count - on lattices that exercise every block shape and on fields that exercise the inside rule, long parent chains and the
selection; poisoned outputs and workspace with guard rows, in-place calls, a recorded call; the Python entry points and the composer
(``extract_mesh`` / ``build_occupancy`` with the new keywords) on the small tennis networks."""
import ctypes as C

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, occupancy, surface
from tests import components_reference as cr
from tests import surface_reference as sr
from tests.test_gpu import ATOL, RTOL
from tests.test_surface_gpu import PLAYER_1, codes, tennis

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 64           # int32 values behind every output and behind the workspace that must stay poisoned
LATTICES = [(1, 1, 1), (2, 2, 2), (1, 1, 300), (2, 2, 300), (5, 6, 7), (9, 17, 33), (16, 16, 17)]
SHAPE = (9, 17, 33)
FIELDS = ("two_blob", "torus", "noise_0.5", "noise_0.75", "noise_0.85", "equal_to_level", "all_inside", "all_outside", "non_finite", "comb")
OUTPUTS = ("labels", "sizes", "sigma_out")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# fields and helpers
def make_field(kind, shape, seed=0):
    """(field (nx, ny, nz) fp32, level)."""
    axes = [np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    if kind == "two_blob":                     # tests/components_reference.two_blob_field on a lattice that is not a cube
        f = np.maximum(0.25 - (X + 0.3) ** 2 - Y ** 2 - Z ** 2, 0.04 - (X - 0.7) ** 2 - (Y - 0.6) ** 2 - (Z - 0.6) ** 2).astype(np.float32)
        for at in ((1, 1, 1), (nx - 2, 1, 2), (nx - 3, 2, 3), (1, ny - 2, 1), (2, ny - 1, 2)):
            f[at] = 1.0
        return f, 0.0
    if kind == "torus":
        return (0.23 ** 2 - (np.sqrt(X * X + Y * Y) - 0.55) ** 2 - Z * Z).astype(np.float32), 0.0
    if kind.startswith("noise"):
        return rng.uniform(0, 1, shape).astype(np.float32), float(kind.split("_")[1]) if "_" in kind else 0.5
    if kind == "equal_to_level":           # a third of the entries sit exactly on the level: they are outside
        return rng.integers(-1, 2, shape).astype(np.float32) * 0.5 + 0.25, 0.25
    if kind == "all_inside":
        return np.full(shape, 3.0, dtype=np.float32), 0.0
    if kind == "all_outside":
        return np.full(shape, -3.0, dtype=np.float32), 0.0
    if kind == "non_finite":
        f = rng.uniform(-1, 1, shape).astype(np.float32)
        pick = rng.uniform(0, 1, shape)
        f[pick < 0.06] = np.nan
        f.view(np.int32)[pick < 0.02] = 0x7FC12345          # ... some of them with a payload
        f[(pick >= 0.06) & (pick < 0.10)] = np.inf
        f[(pick >= 0.10) & (pick < 0.14)] = -np.inf
        return f, 0.0
    if kind == "comb":                      # teeth along z on every other (i, j), joined only by the far plane k = nz - 1: one component
        f = np.full(shape, -1.0, dtype=np.float32)          # whose root, point 0, is as far from the joints as the lattice allows
        f[::2, ::2, :] = 1.0
        f[:, :, nz - 1] = 1.0
        return f, 0.0
    raise KeyError(kind)


def stack(shape, kinds, seed=0, level=None):
    """(sigma (G, ...), level): one field per group, shifted to a common level (default: the first field's own)."""
    fields = []
    for g, kind in enumerate(kinds):
        f, lv = make_field(kind, shape, seed=seed + g)
        level = lv if level is None else level
        fields.append(f + np.float32(level - lv) if lv != level else f)
    return np.stack(fields), level


_REFERENCE = {}


def reference(key, sigma, level, **options):
    """The reference result of a case, computed once and never modified."""
    key = (key, level, tuple(sorted(options.items())))
    if key not in _REFERENCE:
        _REFERENCE[key] = cr.clean(sigma, level, **options)
    return _REFERENCE[key]


def poisoned(count):
    return torch.full((count,), POISON, dtype=torch.int32, device="cuda")


def run_abi(sigma, level, outputs=OUTPUTS, in_place=False, check=True, **options):
    """One ``pr_label_components`` call on poisoned outputs and a poisoned workspace, each followed by guard values.  Returns the
    outputs as int32 CPU tensors of the lattice's shape (``sigma_out``: the bit patterns), ``counts`` and the status."""
    lib = _lib.load()
    dev_sigma = torch.as_tensor(np.ascontiguousarray(sigma, dtype=np.float32)).cuda()
    total = dev_sigma.numel()
    buffers = {name: poisoned(total + GUARD) for name in outputs}
    if in_place:
        buffers["sigma_out"] = poisoned(total + GUARD)
        buffers["sigma_out"][:total] = dev_sigma.view(torch.int32).reshape(-1)
        dev_sigma = buffers["sigma_out"][:total].view(torch.float32).reshape(dev_sigma.shape)
    counts = poisoned(dev_sigma.size(0) * 4 + GUARD)
    c = surface.components_struct(dev_sigma, level, counts, **{name: buffers.get(name) for name in OUTPUTS}, **options)
    size = C.c_size_t()
    status = lib.pr_components_workspace_size(C.byref(c), C.byref(size))
    workspace = None
    if status == 0:
        workspace = poisoned(size.value // 4 + GUARD)
        status = lib.pr_label_components(C.byref(c), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if check:
        _lib.check(status, "pr_label_components")
    got = {"status": status, "counts": counts[:-GUARD].reshape(-1, 4).cpu()}
    for name, t in buffers.items():
        assert bool((t[total:] == POISON).all()), f"{name}: written behind its end"
        got[name] = t[:total].reshape(dev_sigma.shape).cpu()
    assert bool((counts[-GUARD:] == POISON).all()), "counts: written behind its end"
    if workspace is not None:
        assert bool((workspace[size.value // 4:] == POISON).all()), "workspace: written behind its end"
    return got


def assert_equals_reference(got, want, what):
    assert torch.equal(got["counts"], torch.from_numpy(want["counts"])), (what, got["counts"].tolist(), want["counts"].tolist())
    for name in ("labels", "sizes"):
        if name in got:
            assert torch.equal(got[name], torch.from_numpy(want[name])), (what, name)
    if "sigma_out" in got:
        assert torch.equal(got["sigma_out"], torch.from_numpy(cr.bits(want["sigma_out"]))), (what, "sigma_out")


# ---------------------------------------------------------------------------------------------------------------------
# 1. labels, sizes, counts and sigma_out through the C ABI
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("shape", LATTICES, ids=["x".join(map(str, s)) for s in LATTICES])
def test_lattices_equal_the_reference(shape, groups):
    kinds = ["noise_0.5"] if groups == 1 else ["noise_0.5", "torus", "non_finite"]
    sigma, level = stack(shape, kinds)
    for close_border in (True, False):
        want = reference(("lattice", shape, groups), sigma, level, close_border=close_border, min_points=2)
        got = run_abi(sigma, level, close_border=close_border, min_points=2)
        assert_equals_reference(got, want, (shape, groups, close_border))
    print(f"{shape} G={groups}: counts {want['counts'].tolist()}")
    assert want["counts"][0, 0] > 0                              # the noise group has inside points on every lattice


def test_one_long_component_is_one_label():
    """(2, 2, 300), every point inside: one component of 1200 points across five blocks - a long chain of parents."""
    sigma = np.full((1, 2, 2, 300), 1.0, dtype=np.float32)
    got = run_abi(sigma, 0.0)
    assert got["counts"].tolist() == [[1200, 1, 1, 1200]]
    assert bool((got["labels"] == 0).all()) and bool((got["sizes"] == 1200).all())
    assert_equals_reference(got, reference("long", sigma, 0.0), "long")


NOISE_COMPONENTS = {"noise_0.5": 3, "noise_0.75": 92, "noise_0.85": 235}       # what the reference finds in default_rng(0).uniform(0, 1)


@pytest.mark.parametrize("kind", FIELDS)
def test_fields_equal_the_reference(kind):
    f, level = make_field(kind, SHAPE)
    sigma = f[None]
    want = reference(("field", kind), sigma, level)
    got = run_abi(sigma, level)
    assert_equals_reference(got, want, kind)
    inside, components = want["counts"][0, :2].tolist()
    print(f"{kind}: {inside} inside points, {components} components, largest {int(want['sizes'].max())}")
    P = int(np.prod(SHAPE))
    if kind == "all_inside":
        assert got["counts"].tolist() == [[P, 1, 1, P]]
    elif kind == "all_outside":
        assert got["counts"].tolist() == [[0, 0, 0, 0]] and bool((got["labels"] == -1).all()) and bool((got["sizes"] == 0).all())
    elif kind == "comb":
        assert components == 1 and bool((got["labels"][got["labels"] >= 0] == 0).all())
    elif kind == "two_blob":
        assert components == 6
    elif kind == "torus":
        assert components == 1
    elif kind in NOISE_COMPONENTS:
        assert components == NOISE_COMPONENTS[kind]
    elif kind == "equal_to_level":
        assert bool((got["labels"][torch.from_numpy(f[None] == np.float32(level))] == -1).all())
    elif kind == "non_finite":
        assert bool((got["labels"][torch.from_numpy(np.isnan(f[None]))] == -1).all())
        assert bool((got["labels"][torch.from_numpy(np.isposinf(f[None]))] >= 0).all())
        assert np.isnan(want["sigma_out"]).sum() == np.isnan(f).sum() > 0
    # with the border closed, and everything but the largest component blanked out
    want = reference(("field", kind), sigma, level, close_border=True, keep_largest=1, fill=-1.0)
    assert_equals_reference(run_abi(sigma, level, close_border=True, keep_largest=1, fill=-1.0), want, (kind, "closed"))


def test_groups_with_different_fields_and_empty_groups():
    sigma, level = stack(SHAPE, ["torus", "all_outside", "noise_0.75", "all_outside", "two_blob"], seed=5)
    want = reference("five groups", sigma, level, keep_largest=2)
    got = run_abi(sigma, level, keep_largest=2)
    assert_equals_reference(got, want, "five groups")
    counts = got["counts"].tolist()
    assert counts[1] == counts[3] == [0, 0, 0, 0] and counts[0][1:3] == [1, 1] and counts[2][2] == 2 and counts[4][1:3] == [6, 2]


# ---------------------------------------------------------------------------------------------------------------------
# 2. selection
def selection_case():
    return stack(SHAPE, ["two_blob", "noise_0.75", "noise_0.85"], seed=0)


@pytest.mark.parametrize("keep_largest", [0, 1, 2, 8])
@pytest.mark.parametrize("min_points", [0, 2, 18])
def test_selection_equals_the_reference(min_points, keep_largest):
    sigma, level = selection_case()
    want = reference("selection", sigma, level, min_points=min_points, keep_largest=keep_largest)
    got = run_abi(sigma, level, min_points=min_points, keep_largest=keep_largest)
    assert_equals_reference(got, want, (min_points, keep_largest))
    print(f"min_points {min_points}, keep_largest {keep_largest}: counts {want['counts'].tolist()}")
    if keep_largest:
        assert all(row[2] <= keep_largest for row in got["counts"].tolist())
    if not min_points and not keep_largest:
        assert torch.equal(got["sigma_out"], torch.from_numpy(cr.bits(sigma)))          # everything kept: a copy


def test_ties_in_size_go_to_the_smaller_label():
    """Six single points and two pairs: ranks 0 and 1 are the pairs, the singles follow by label."""
    sigma = np.zeros((1, 5, 6, 7), dtype=np.float32)
    singles = [(4, 5, 6), (0, 0, 0), (2, 3, 0), (0, 5, 3), (4, 0, 3), (2, 0, 6)]
    for at in singles + [(1, 2, 2), (2, 3, 3), (3, 1, 4), (3, 1, 5)]:
        sigma[0][at] = 1.0
    flat = lambda at: (at[0] * 6 + at[1]) * 7 + at[2]
    for keep in range(1, 9):
        got = run_abi(sigma, 0.5, keep_largest=keep, fill=0.0)
        assert_equals_reference(got, reference("ties", sigma, 0.5, keep_largest=keep, fill=0.0), keep)
        kept = sorted(set(got["labels"][got["sigma_out"] != 0].tolist()))
        want = sorted([flat((1, 2, 2)), flat((3, 1, 4))][:keep] + sorted(flat(s) for s in singles)[:max(0, keep - 2)])
        assert kept == want, (keep, kept, want)
        assert got["counts"].tolist() == [[10, 8, keep, min(keep, 2) * 2 + max(0, keep - 2)]]


# ---------------------------------------------------------------------------------------------------------------------
# 3. flags and outputs
@pytest.mark.parametrize("fill", ["level", -1.0, float("-inf")], ids=["level", "minus_one", "minus_inf"])
@pytest.mark.parametrize("close_border", [False, True], ids=["open", "closed"])
def test_close_border_and_fill(close_border, fill):
    sigma, level = stack(SHAPE, ["two_blob", "non_finite", "all_inside"], seed=2)
    options = dict(close_border=close_border, min_points=3, fill=None if fill == "level" else fill)
    want = reference("flags", sigma, level, **options)
    got = run_abi(sigma, level, **options)
    assert_equals_reference(got, want, (close_border, fill))
    if close_border:
        border = np.ones(SHAPE, dtype=bool)
        border[1:-1, 1:-1, 1:-1] = False
        assert bool((got["labels"][:, torch.from_numpy(border)] == -1).all())
        value = np.float32(level if fill == "level" else fill)
        assert bool((got["sigma_out"][2][torch.from_numpy(border)] == int(cr.bits(value).reshape(-1)[0])).all())       # the all-inside group is capped


def test_in_place_equals_out_of_place():
    sigma, level = stack(SHAPE, ["two_blob", "non_finite", "noise_0.75"], seed=4)
    options = dict(close_border=True, keep_largest=2, fill=-2.0)
    want = reference("in place", sigma, level, **options)
    assert_equals_reference(run_abi(sigma, level, in_place=True, **options), want, "in place")
    assert_equals_reference(run_abi(sigma, level, outputs=(), in_place=True, **options), want, "in place, alone")


@pytest.mark.parametrize("output", [None, "labels", "sizes", "sigma_out"])
def test_each_output_alone(output):
    sigma, level = stack(SHAPE, ["two_blob", "non_finite", "noise_0.75"], seed=4)
    options = dict(min_points=2, keep_largest=8)
    want = reference("alone", sigma, level, **options)
    got = run_abi(sigma, level, outputs=() if output is None else (output,), **options)
    assert set(got) == {"status", "counts"} | ({output} if output else set())
    assert_equals_reference(got, want, output)


# ---------------------------------------------------------------------------------------------------------------------
# 4. robustness
def test_two_runs_are_identical():
    sigma, level = stack((16, 16, 17), ["noise_0.5", "noise_0.75", "comb"], seed=9)
    a = run_abi(sigma, level, keep_largest=3, min_points=2)
    b = run_abi(sigma, level, keep_largest=3, min_points=2)
    for name in OUTPUTS + ("counts",):
        assert torch.equal(a[name], b[name]), name


def test_a_recorded_call_holds_kernels_only_and_replays_on_new_lattices():
    keep = 2
    cases = [stack(SHAPE, kinds, seed=s, level=0.5) for kinds, s in ((["noise_0.5", "torus", "non_finite"], 0), (["comb", "noise_0.5", "two_blob"], 7),
                                                          (["all_outside", "all_inside", "noise_0.5"], 3))]
    assert all(level == 0.5 for _, level in cases)
    lib = _lib.load()
    G, total = 3, 3 * int(np.prod(SHAPE))
    sigma = torch.from_numpy(cases[0][0]).cuda()
    out = {name: poisoned(total) for name in OUTPUTS}
    counts = poisoned(G * 4)
    c = surface.components_struct(sigma, 0.5, counts, labels=out["labels"], sizes=out["sizes"], sigma_out=out["sigma_out"], keep_largest=keep,
                                  close_border=True, fill=0.0)
    size = C.c_size_t()
    _lib.check(lib.pr_components_workspace_size(C.byref(c), C.byref(size)), "pr_components_workspace_size")
    workspace = poisoned(size.value // 4)
    run = lambda: _lib.check(lib.pr_label_components(C.byref(c), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream),
                             "pr_label_components")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    census = frame_graph.node_census(graph)
    print("recorded labelling:", census)
    assert census == {"nodes": 4 + keep, "kernels": 4 + keep, "memsets": 0, "memcpys": 0}
    graph.instantiate()
    for index in (1, 0, 2, 1):
        sig, level = cases[index]
        sigma.copy_(torch.from_numpy(sig))
        for t in list(out.values()) + [counts, workspace]:
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        got = {name: t.reshape(sigma.shape).cpu() for name, t in out.items()}
        got["counts"] = counts.reshape(G, 4).cpu()
        assert_equals_reference(got, reference(("replay", index), sig, level, keep_largest=keep, close_border=True, fill=0.0), ("replay", index))


@pytest.mark.parametrize("options,message", [(dict(keep_largest=9), "keep_largest 9"), (dict(min_points=-1), "min_points -1"),
                                             (dict(fill=1.0), "must be <= level"), (dict(fill=float("nan")), "must be <= level")])
def test_refusals_leave_the_outputs_alone(options, message):
    sigma, level = stack((5, 6, 7), ["noise_0.5"])
    got = run_abi(sigma, level, check=False, **options)
    assert got["status"] == -1 and message in _lib.load().pr_last_error().decode()
    for name in OUTPUTS + ("counts",):
        assert bool((got[name] == POISON).all()), name


# ---------------------------------------------------------------------------------------------------------------------
# 5. the python entry points
def test_label_components_and_clean_lattice_equal_the_reference():
    sigma, level = stack(SHAPE, ["two_blob", "non_finite", "noise_0.75"], seed=4)
    dev = torch.from_numpy(sigma).cuda()
    for close_border in (False, True):
        want = reference("python", sigma, level, close_border=close_border)
        labels, sizes, counts = surface.label_components(dev, level, close_border=close_border)
        assert labels.is_cuda and labels.dtype == sizes.dtype == counts.dtype == torch.int32 and list(counts.shape) == [3, 4]
        assert_equals_reference({"labels": labels.cpu(), "sizes": sizes.cpu(), "counts": counts.cpu()}, want, close_border)
    for options in (dict(keep_largest=1), dict(min_points=3, close_border=True, fill=-1.0), dict(keep_largest=8, min_points=2, fill=float("-inf"))):
        want = reference("python", sigma, level, **options)
        out, counts = surface.clean_lattice(dev, level, **options)
        assert out.is_cuda and out.dtype == torch.float32 and out.data_ptr() != dev.data_ptr()
        assert_equals_reference({"sigma_out": out.view(torch.int32).cpu(), "counts": counts.cpu()}, want, options)
    assert torch.equal(dev.view(torch.int32).cpu(), torch.from_numpy(cr.bits(sigma)))                # the input is never touched
    with pytest.raises(RuntimeError, match="keep_largest 9"):                                       # the library's refusal surfaces
        surface._run_components(dev, level, keep_largest=9)


def test_extract_surface_cleans_the_lattice_first():
    fields = [cr.two_blob_field(17)[0], sr.sphere_field(17, r=1.2)[0], sr.torus_field(17)[0]]
    axes = cr.two_blob_field(17)[1]
    sigma = np.stack(fields)
    dev, dev_axes = torch.from_numpy(sigma).cuda(), [torch.from_numpy(a).cuda() for a in axes]
    plain = surface.extract_surface(dev, dev_axes, 0.0)
    for options in (dict(keep_largest=1), dict(close_border=True), dict(min_points=3, keep_largest=2, close_border=True)):
        cleaned = torch.from_numpy(reference("extract", sigma, 0.0, **options)["sigma_out"]).cuda()
        want = surface.extract_surface(cleaned, dev_axes, 0.0)
        got = surface.extract_surface(dev, dev_axes, 0.0, **options)
        assert len(got) == len(want) == 3
        for g in range(3):
            assert torch.equal(got[g].vertices, want[g].vertices) and torch.equal(got[g].triangles, want[g].triangles), (options, g)
            assert torch.equal(got[g].normals, want[g].normals), (options, g)
        if options == dict(keep_largest=1):
            assert (got[0].vertices.size(0), got[0].triangles.size(0)) == (890, 1776)
            assert (plain[0].vertices.size(0), plain[0].triangles.size(0)) == (1090, 2152)
            rows = {bytes(r) for r in plain[0].vertices.cpu().numpy()}
            assert all(bytes(r) in rows for r in got[0].vertices.cpu().numpy())
            assert torch.equal(got[2].vertices, plain[2].vertices)                       # one component: nothing to remove
        if options == dict(close_border=True):
            assert (got[1].vertices.size(0), got[1].triangles.size(0)) == (4490, 8976)
            assert sr.directed_edges_once(got[1].triangles.cpu().numpy()) and not sr.directed_edges_once(plain[1].triangles.cpu().numpy())
    default = surface.extract_surface(dev, dev_axes, 0.0, keep_largest=0, min_points=0, close_border=False)
    for g in range(3):
        assert torch.equal(default[g].vertices, plain[g].vertices) and torch.equal(default[g].triangles, plain[g].triangles)
        assert torch.equal(default[g].normals, plain[g].normals)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the composer
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_extract_mesh_with_the_largest_component_and_a_closed_border(precision):
    cfg, comp = tennis(precision)
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, centres = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        meshes = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, keep_largest=1, close_border=True)
        plain = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level)
        default = comp.extract_mesh(PLAYER_1, 24, style, deformation, level=level, keep_largest=0, min_points=0, close_border=False)
    axes = [centres[:, 0, 0, 0].cpu().numpy(), centres[0, :, 0, 1].cpu().numpy(), centres[0, 0, :, 2].cpu().numpy()]
    cleaned = cr.clean(sigma.cpu().numpy(), level, keep_largest=1, close_border=True)
    want = sr.extract_surface(cleaned["sigma_out"], axes, level)
    vo, to = want["vertex_offsets"], want["triangle_offsets"]
    print(f"{precision}: level {level:.4g}, counts {cleaned['counts'].tolist()}, V {vo.tolist()}, T {to.tolist()}, "
          f"uncleaned V {[m.vertices.size(0) for m in plain]}")
    assert len(meshes) == 2 and vo[1] > 0 and vo[2] > vo[1]
    assert (cleaned["counts"][:, 2] == 1).all()
    for g, m in enumerate(meshes):
        assert torch.equal(m.vertices.cpu(), torch.from_numpy(want["vertices"][vo[g]:vo[g + 1]]))
        assert torch.equal(m.triangles.cpu(), torch.from_numpy(want["triangles"][to[g]:to[g + 1]]))
        assert torch.allclose(m.normals.cpu(), torch.from_numpy(want["normals"][vo[g]:vo[g + 1]]), rtol=RTOL, atol=ATOL)
        assert sr.directed_edges_once(m.triangles.cpu().numpy())                          # one capped component: a closed mesh
        assert torch.equal(default[g].vertices, plain[g].vertices) and torch.equal(default[g].triangles, plain[g].triangles)
        assert torch.equal(default[g].normals, plain[g].normals)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_build_occupancy_without_the_floaters(precision):
    cfg, comp = tennis(precision)
    style, deformation = codes(cfg)
    K = comp.object_id_helper.objects_count
    res, ss, dil = 12, 2, 0
    sty = torch.zeros(2, style.size(1), K, device="cuda")
    dfm = torch.zeros(2, deformation.size(1), K, device="cuda")
    sty[..., PLAYER_1], dfm[..., PLAYER_1] = style, deformation
    with torch.no_grad():
        thr = float(comp.density_grid(PLAYER_1, res * ss, style, deformation)[0].median())
        args = dict(resolution=res, supersample=ss, threshold=thr, dilate=dil, objects=[PLAYER_1])
        occ = comp.build_occupancy(sty, dfm, keep_largest=1, **args)
        plain = comp.build_occupancy(sty, dfm, **args)
        default = comp.build_occupancy(sty, dfm, keep_largest=0, min_points=0, **args)
        assert set(occ.grids) == set(plain.grids) == {(PLAYER_1, "coarse"), (PLAYER_1, "fine")}
        for (k, level), g in occ.grids.items():
            sigma, _ = comp.density_grid(k, res * ss, style, deformation, fine=level == "fine")
            cleaned = cr.clean(sigma.cpu().numpy(), thr, keep_largest=1, fill=thr)
            want = torch.full_like(g["bits"], POISON)
            lattice = torch.from_numpy(cleaned["sigma_out"]).cuda()
            _lib.check(_lib.load().pr_occupancy_build(lattice.data_ptr(), 2, (C.c_int32 * 3)(res, res, res), ss,
                                                      thr, dil, want.data_ptr(), torch.cuda.current_stream().cuda_stream), "pr_occupancy_build")
            torch.cuda.synchronize()
            assert torch.equal(g["bits"], want), (k, level)
            assert torch.equal(default.grids[(k, level)]["bits"], plain.grids[(k, level)]["bits"]), (k, level)
            before = int(occupancy.unpack_bits(plain.grids[(k, level)]["bits"], g["cells"]).sum())
            after = int(occupancy.unpack_bits(g["bits"], g["cells"]).sum())
            print(f"{precision} {level}: components {cleaned['counts'][:, 1].tolist()}, occupied cells {before} -> {after}")
            assert after <= before                                                        # cleaning only ever frees cells
        before = {key: g["bits"].clone() for key, g in occ.grids.items()}
        for g in occ.grids.values():
            g["bits"].fill_(POISON)
        occ.update(sty, dfm)                     # an update cleans the same way
        for key, g in occ.grids.items():
            assert torch.equal(g["bits"], before[key]), key
    with pytest.raises(ValueError):
        comp.build_occupancy(sty, dfm, keep_largest=9, **args)

"""Smoothing on the GPU (python -m pytest tests -m gpu): ``pr_mesh_smooth`` against its numpy restatement (tests/smooth_reference.py) -
positions, normals, both CSR arrays, state and counts on their 32-bit words, and equal bits from call to call - through the C ABI on
poisoned outputs and a poisoned workspace with guard rows behind every array; hand-made meshes, the welded test meshes in one group and
in three, groups at the seams of the blocks and one above 256 x 256 vertices, ``max_degree`` below the largest k, both parities of the
buffer alternation, the factors, the border flag and a mask, every optional output, empty and hostile input, a recorded call replayed
on another mesh, the consumers (audit, contains, distance_to), the Python layer, ``extract_surface(smooth=n)`` and
``ObjectComposer.extract_mesh(smooth=n)`` on the small tennis networks."""
import ctypes as C

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, surface
from tests import inside_reference as ir
from tests import smooth_reference as sm
from tests import surface_reference as sr
from tests import weld_reference as wr
from tests.test_raycast_gpu import device_mesh, hostile, to_meshes
from tests.test_surface_gpu import GUARD, PLAYER_1, POISON, codes, is_poison, make_field, poisoned, tennis
from tests.test_weld_gpu import level_lattice_capped, sliced_sphere

pytestmark = pytest.mark.gpu

F = np.float32
KERNELS = 9                        # the header's launch count with steps == 0; one more per step
KINDS = ("sphere", "torus", "plane", "noise", "capped_noise", "simplified_kept")
OUTPUTS = ("out_normals", "csr", "vertex_state")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes and references (numpy only), computed once
_WELDED, _REFERENCES = {}, {}


def welded(kind, groups=1):
    """The packed, welded mesh of one of ``inside_reference.MESHES`` in one group, or in three."""
    if (kind, groups) not in _WELDED:
        _WELDED[(kind, groups)] = wr.weld(ir.mesh_case(kind, groups)[0])
    return _WELDED[(kind, groups)]


def plain(mesh):
    return {key: mesh[key] for key in ("vertices", "triangles", "vertex_offsets", "triangle_offsets", "V", "T") if key in mesh}


def reference(key, mesh, **kw):
    """``sm.smooth`` of a shared case, computed once (``key`` None: not kept)."""
    pinned = kw.get("pinned")
    full = None if key is None or pinned is not None else (key,) + tuple(sorted(kw.items()))
    if full is None:
        return sm.smooth(plain(mesh), **kw)
    if full not in _REFERENCES:
        _REFERENCES[full] = sm.smooth(plain(mesh), **kw)
    return _REFERENCES[full]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on poisoned memory
def allocate(V, T, G, outputs):
    """Poisoned outputs with guard rows: ``(tensors, rows, shapes)``."""
    out = {"out_vertices": poisoned(((V + GUARD) * 3,), torch.float32), "counts": poisoned((G * 8 + GUARD,), torch.int32)}
    rows = {"out_vertices": V * 3, "counts": G * 8}
    shapes = {"out_vertices": (V, 3), "counts": (G, 8)}
    if "out_normals" in outputs:
        out["out_normals"], rows["out_normals"], shapes["out_normals"] = poisoned(((V + GUARD) * 3,), torch.float32), V * 3, (V, 3)
    if "csr" in outputs:
        out["incidence_offsets"], rows["incidence_offsets"], shapes["incidence_offsets"] = poisoned((V + 1 + GUARD,), torch.int32), V + 1, (V + 1,)
        out["incidence"], rows["incidence"], shapes["incidence"] = poisoned((3 * T + GUARD,), torch.int32), 3 * T, (3 * T,)
    if "vertex_state" in outputs:
        out["vertex_state"], rows["vertex_state"], shapes["vertex_state"] = poisoned((V + GUARD,), torch.int32), V, (V,)
    return out, rows, shapes


def run_smooth(dev, steps=0, lam=0.5, mu=-0.53, max_degree=64, flags=1, pinned=None, outputs=OUTPUTS):
    """One call on poisoned outputs and a poisoned workspace, guard rows behind every array.  Returns the outputs without their
    guards (which are checked here)."""
    G, V, T = dev["vertex_offsets"].numel() - 1, dev["V"], dev["T"]
    out, rows, shapes = allocate(V, T, G, outputs)
    mask = None if pinned is None or V == 0 else cuda(np.asarray(pinned, dtype=np.uint8))
    s = surface.smooth_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], V, T, out["out_vertices"],
                              out["counts"], steps=steps, lam=lam, mu=mu, max_degree=max_degree, pin_border=bool(flags & 1), pinned=mask,
                              **{k: t for k, t in out.items() if k not in ("out_vertices", "counts")})
    size = C.c_size_t()
    lib = _lib.load()
    _lib.check(lib.pr_mesh_smooth_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_smooth_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")          # (64 guard words)
    _lib.check(lib.pr_mesh_smooth(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream), "pr_mesh_smooth")
    torch.cuda.synchronize()
    assert bool(is_poison(workspace[size.value // 4:]).all()), "workspace guard"
    for key, t in out.items():
        assert bool(is_poison(t[rows[key]:]).all()), ("guard", key)
    return {key: t[:rows[key]].reshape(shapes[key]) for key, t in out.items()}


REFERENCE_KEYS = {"out_vertices": "vertices", "out_normals": "normals", "incidence_offsets": "incidence_offsets", "incidence": "incidence",
                  "vertex_state": "state", "counts": "counts"}


def sort_long_lists(entries, want, max_degree):
    """``entries`` (numpy, the written ones) with the segments of the vertices with k > max_degree sorted: their order is unspecified."""
    entries = entries.copy()
    offsets = want["incidence_offsets"]
    for v in np.nonzero(want["k"] > max_degree)[0].tolist():
        entries[offsets[v]:offsets[v + 1]] = np.sort(entries[offsets[v]:offsets[v + 1]])
    return entries


def assert_smooth_equal(got, want, what, max_degree=64):
    """Every output on its 32-bit words (floats are compared as bits: the sign of zero counts; inputs are finite apart from
    designated vertices, which are copied, so no NaN is computed).  ``incidence``: the written entries are the reference's, the
    segments of over-degree vertices as sorted sets; behind the total nothing is written."""
    for key, t in got.items():
        expected = cuda(want[REFERENCE_KEYS[key]]).view(torch.int32)
        if key == "incidence":
            total = int(want["incidence_offsets"][-1])
            assert expected.numel() == total and bool(is_poison(t[total:]).all()), (what, key, "behind the total")
            t = t[:total]
            if (want["k"] > max_degree).any():
                t = cuda(sort_long_lists(t.cpu().numpy(), want, max_degree))
        expected = expected.reshape(t.shape) if expected.numel() == t.numel() else expected
        assert expected.shape == t.shape, (what, key, expected.shape, t.shape)
        wrong = t.view(torch.int32) != expected
        assert not bool(wrong.any()), (what, key, int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())


def check_case(mesh, key, what=None, again=True, outputs=OUTPUTS, **kw):
    """The call with every output against the reference, and a second call into fresh buffers against the first."""
    want = reference(key, mesh, **kw)
    dev = device_mesh(plain(mesh))
    got = run_smooth(dev, outputs=outputs, **kw)
    max_degree = kw.get("max_degree", 64)
    assert_smooth_equal(got, want, what or key, max_degree)
    if again:
        second = run_smooth(dev, outputs=outputs, **kw)
        for name in got:
            a, b = got[name], second[name]
            if name == "incidence" and (want["k"] > max_degree).any():
                total = int(want["incidence_offsets"][-1])
                a, b = (cuda(sort_long_lists(x[:total].cpu().numpy(), want, max_degree)) for x in (a, b))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what or key, name)
    return got, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. identity through the C ABI
def test_hand_made_meshes():
    cases = (("tetrahedron", sm.tetrahedron()), ("triangle", sm.one_triangle()), ("hexagon", sm.fan(6)), ("open fan", sm.fan(6, closed=False)),
             ("fan 64", sm.fan(64)), ("fan 65", sm.fan(65)), ("broken", sm.broken()),
             ("fan 1100", sm.fan(1100)))                                # (a list behind the 1023 positions that the count keeps)
    for name, mesh in cases:
        for kw in (dict(steps=0), dict(steps=1, lam=1.0, mu=1.0), dict(steps=4), dict(steps=3, flags=0)):
            got, want = check_case(mesh, None, what=(name, kw), again=kw["steps"] == 4, **kw)
        print(name, want["counts"].tolist())
    got, _ = check_case(sm.tetrahedron(), None, steps=1, lam=1.0, mu=1.0)
    third = float(F(2) / F(6))
    assert got["out_vertices"].tolist() == [[third] * 3, [0, third, third], [third, 0, third], [third, third, 0]]
    assert got["counts"].tolist() == [[4, 0, 4, 0, 0, 0, 0, 3]] and got["incidence"].tolist() == [0, 1, 3, 0, 1, 2, 0, 2, 3, 1, 2, 3]
    got, _ = check_case(sm.fan(65), None, steps=1)
    assert got["counts"].tolist() == [[65, 0, 0, 0, 65, 1, 0, 65]] and got["vertex_state"][0].item() == 9 and not got["out_normals"][0].any()
    got, _ = check_case(sm.fan(64), None, steps=1)
    assert got["counts"].tolist() == [[64, 0, 1, 0, 64, 0, 0, 64]] and got["vertex_state"][0].item() == 33


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_smooth_equals_the_reference_and_repeats_bit_for_bit(kind, groups):
    mesh = welded(kind, groups)
    got, want = check_case(mesh, (kind, groups), steps=4)
    counts = want["counts"]
    print(f"{kind} G={groups}: V {mesh['vertex_offsets'].tolist()} T {mesh['triangle_offsets'].tolist()} counts {counts.tolist()}")
    assert np.array_equal(counts[:, 0] + counts[:, 1], np.diff(mesh["triangle_offsets"])) and (counts[:, 2] > 0).all()
    assert not torch.equal(got["out_vertices"], cuda(mesh["vertices"]))          # something moved
    check_case(mesh, (kind, groups), steps=0, again=False)


def test_the_recorded_answers():
    for kind, largest, border in (("sphere", 8, 0), ("torus", 9, 0), ("plane", 8, 36), ("noise", 10, 2662), ("capped_noise", 10, 0),
                                  ("simplified_kept", 10, 0)):
        got = run_smooth(device_mesh(plain(welded(kind))))
        assert got["counts"][0, [7, 4]].tolist() == [largest, border], kind
    got, _ = check_case(welded("equal_to_level"), ("equal_to_level", 1), again=False)
    assert got["counts"][0].tolist()[:2] == [18411, 21864 - 18411] and got["counts"][0, 7].item() == 24 and got["counts"][0, 3].item() == 1
    sphere = welded("sphere")
    got, _ = check_case(sphere, ("sphere", 1), again=False)
    assert torch.equal(got["out_vertices"].view(torch.int32), cuda(sphere["vertices"]).view(torch.int32))      # steps == 0: a copy
    dots = (got["out_normals"] * cuda(ir.part("sphere")[0]["normals"])).sum(dim=1)
    assert float(dots.min()) > 0.98


# ---------------------------------------------------------------------------------------------------------------------
# 2. block seams, the scan's upper level, max_degree
def test_groups_at_the_seams_of_the_blocks():
    sizes = [(255, 255), (256, 256), (257, 257), (513, 513), (255, 513), (513, 255), (256, 257), (1, 1), (257, 256)]
    mesh = sliced_sphere(sizes)
    assert np.diff(mesh["vertex_offsets"]).tolist() == [s[0] for s in sizes] and np.diff(mesh["triangle_offsets"]).tolist() == [s[1] for s in sizes]
    for kw in (dict(steps=3), dict(steps=2, flags=0)):
        got, want = check_case(mesh, "seams", **kw)
    counts = want["counts"]
    print("seams:", counts.tolist())
    assert (counts[:, 1] > 0).any() and (counts[:, 3] > 0).any() and (counts[:, 2] > 0).sum() >= 6 and counts[7].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]


def test_one_group_above_256_x_256_vertices():
    n = 33
    field = np.random.default_rng(5).integers(-1, 2, (n, n, n)).astype(F) * F(0.5) + F(0.25)
    mesh = wr.weld(ir.pack([sr.extract_surface(field[None], [np.linspace(-1, 1, n).astype(F)] * 3, 0.25, normals=False)]))
    assert len(mesh["vertices"]) == 65970 > 256 * 256
    got, want = check_case(mesh, None, what="33^3", again=False, steps=2)
    print("33^3:", want["counts"].tolist())
    assert int(got["incidence_offsets"][-1]) == 3 * int(got["counts"][0, 0]) > 3 * 256 * 256


@pytest.mark.parametrize("max_degree", [1, 8, 256])
def test_max_degree_on_the_lattice_on_the_level(max_degree):
    mesh = welded("equal_to_level")
    got, want = check_case(mesh, ("equal_to_level", 1), steps=3, max_degree=max_degree)
    counts = got["counts"][0].tolist()
    print(f"max_degree {max_degree}: {counts}")
    assert counts[7] == 24 and (counts[5] > 0) == (max_degree < 24)
    if max_degree == 8:                                                 # over-degree: immovable, no border bit, a zero normal
        over = (got["vertex_state"] & 8) != 0
        assert int(over.sum()) == counts[5] and not bool((got["vertex_state"][over] & (2 | 32)).any()) and not bool(got["out_normals"][over].any())
        assert torch.equal(got["out_vertices"][over], cuda(mesh["vertices"])[over])


# ---------------------------------------------------------------------------------------------------------------------
# 3. parameters
@pytest.mark.parametrize("steps", [0, 1, 2, 3, 21])
def test_steps_of_both_parities_and_the_factors(steps):
    mesh = welded("torus", 3)
    for lam, mu in ((0.5, -0.53), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (1.0, -0.53), (-0.25, 0.75)):
        got, _ = check_case(mesh, ("torus", 3), again=(lam, mu) == (0.5, -0.53), steps=steps, lam=lam, mu=mu)
        if steps == 0 or (lam, mu) == (0.0, 0.0):
            assert torch.equal(got["out_vertices"].view(torch.int32), cuda(mesh["vertices"]).view(torch.int32))


def test_the_border_flag_and_a_random_mask():
    plane = welded("plane", 3)
    pinned_border, _ = check_case(plane, ("plane", 3), steps=5, flags=1)
    free, _ = check_case(plane, ("plane", 3), steps=5, flags=0)
    border = (free["vertex_state"] & 2) != 0
    assert int(border[:109].sum()) == 36 and torch.equal(free["vertex_state"][:109] & 2, pinned_border["vertex_state"][:109] & 2)
    start = cuda(plane["vertices"])
    assert torch.equal(pinned_border["out_vertices"][border], start[border]) and not torch.equal(free["out_vertices"][border], start[border])
    assert not bool((pinned_border["vertex_state"][border] & 32).any()) and bool((free["vertex_state"][border] & 32).all())
    mesh = welded("noise", 3)
    mask = (np.random.default_rng(7).uniform(0, 1, len(mesh["vertices"])) < 0.3).astype(np.uint8) * 255
    got, want = check_case(mesh, None, what="mask", steps=4, pinned=mask)
    held = cuda(mask != 0)
    assert torch.equal((got["vertex_state"] & 4) != 0, held) and not bool((got["vertex_state"][held] & 32).any())
    assert torch.equal(got["out_vertices"][held], cuda(mesh["vertices"])[held]) and int(got["counts"][:, 2].sum()) < int((~held).sum())


def test_optional_outputs():
    mesh = welded("capped_noise", 3)
    for outputs in (("csr", "vertex_state"), ("out_normals", "vertex_state"), ("out_normals", "csr"), (), ("csr",), ("out_normals",),
                    ("vertex_state",)):
        got, _ = check_case(mesh, ("capped_noise", 3), what=outputs, again=False, outputs=outputs, steps=3)
        assert set(got) == {"out_vertices", "counts"} | ({"out_normals"} & set(outputs)) | ({"vertex_state"} & set(outputs)) | \
            ({"incidence_offsets", "incidence"} if "csr" in outputs else set())


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate input
def test_empty_groups_an_empty_input_and_vertices_without_triangles():
    parts = [wr.weld(ir.pack([ir.part("torus")[0]])), None, wr.weld(ir.pack([ir.part("plane")[0]])), None, wr.weld(ir.pack([ir.part("sphere")[0]]))]
    empty_part = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32)}
    mesh = ir.pack([empty_part if p is None else p for p in parts])
    to = mesh["triangle_offsets"].tolist()
    assert to[1] == to[2] and to[3] == to[4] and to[0] < to[1] < to[3] < to[5]
    got, _ = check_case(mesh, None, what="five groups", steps=3)
    assert not got["counts"][1].any() and not got["counts"][3].any() and int(got["counts"][0, 2]) > 0 and int(got["counts"][4, 2]) > 0
    # an entirely empty input
    empty = {"vertices": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32), "vertex_offsets": np.zeros(3, np.int32),
             "triangle_offsets": np.zeros(3, np.int32)}
    got, _ = check_case(empty, None, what="empty", steps=2)
    assert not got["counts"].any() and got["incidence_offsets"].tolist() == [0]
    # vertices without triangles: finite with k = 0 (or not finite), copied, zero normals
    lone = dict(empty, vertices=np.array([[1, 1, 1], [np.inf, 1, 1], [2, 2, 2], [3, 3, 3], [2, np.nan, 2]], F), vertex_offsets=np.array([0, 2, 5], np.int32))
    got, _ = check_case(lone, None, what="lone", steps=2)
    assert got["counts"].tolist() == [[0, 0, 0, 1, 0, 0, 1, 0], [0, 0, 0, 2, 0, 0, 1, 0]] and got["vertex_state"].tolist() == [0, 16, 0, 0, 16]
    assert torch.equal(got["out_vertices"].view(torch.int32), cuda(lone["vertices"]).view(torch.int32)) and not got["out_normals"].any()


def test_hostile_meshes_and_offsets_cost_correctness_of_their_group_at_most():
    """Randomly broken meshes, and offsets that decrease, leave the arrays or arrive late: guards intact (``run_smooth``), every
    group - the reference clamps as the header says - equal to the reference, and the clean groups' rows equal to the clean meshes'."""
    base = welded("sphere", 3)
    bad = hostile(plain(base))
    V, T = len(base["vertices"]), len(base["triangles"])
    # group 1 of `clean_between` is left as it is: its rows are those of the clean mesh alone
    clean_between = {k: v.copy() for k, v in bad.items()}
    vo, to = base["vertex_offsets"].tolist(), base["triangle_offsets"].tolist()
    clean_between["vertices"][vo[1]:vo[2]] = base["vertices"][vo[1]:vo[2]]
    clean_between["triangles"][to[1]:to[2]] = base["triangles"][to[1]:to[2]]
    got, want = check_case(clean_between, None, what="clean between", steps=3)
    alone = {"vertices": base["vertices"][vo[1]:vo[2]], "triangles": base["triangles"][to[1]:to[2]],
             "vertex_offsets": np.array([0, vo[2] - vo[1]], np.int32), "triangle_offsets": np.array([0, to[2] - to[1]], np.int32)}
    clean = sm.smooth(alone, steps=3)
    assert torch.equal(got["out_vertices"][vo[1]:vo[2]].view(torch.int32), cuda(clean["vertices"]).view(torch.int32))
    assert torch.equal(got["out_normals"][vo[1]:vo[2]].view(torch.int32), cuda(clean["normals"]).view(torch.int32))
    assert torch.equal(got["vertex_state"][vo[1]:vo[2]], cuda(clean["state"])) and got["counts"][1].tolist() == clean["counts"][0].tolist()
    assert int(want["counts"][0, 1]) > 0 and int(want["counts"][0, 6]) > 0 and int(want["counts"][2, 1]) > 0
    cases = [("values", bad)]
    for name, v_off, t_off in (("decreasing", [0, vo[2], vo[1], V], [0, to[2], to[1], T]),
                               ("leaving", [-5, vo[1], V + 1000, 2 ** 31 - 1], [-2 ** 31, to[1], T + 7, T + 9]),
                               ("late", [7, vo[1], vo[2], V - 3], [11, to[1], to[2], T - 5])):
        changed = dict(bad)
        changed["vertex_offsets"], changed["triangle_offsets"] = np.array(v_off, dtype=np.int32), np.array(t_off, dtype=np.int32)
        cases.append((name, changed))
    for name, changed in cases:
        got, want = check_case(changed, None, what=name, again=False, steps=2)
        assert int(want["counts"][:, 1].sum()) > 0 and int(want["counts"][:, 0].sum()) > 0 and int(want["counts"][:, 6].sum()) > 0
        if name == "late":                                             # rows that no clamped group owns: copied, -1, zero normals
            assert got["vertex_state"][:7].tolist() == [-1] * 7 and got["vertex_state"][-3:].tolist() == [-1] * 3
            assert got["incidence_offsets"][:8].tolist() == [0] * 8 and not got["out_normals"][:7].any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a recorded call
@pytest.mark.parametrize("steps", [0, 3])
def test_recorded_call_holds_kernels_only_and_replays_on_a_smaller_mesh_and_back(steps):
    large, small = welded("capped_noise", 3), welded("sphere", 3)
    devs = [device_mesh(plain(large)), device_mesh(plain(small))]
    assert devs[1]["T"] < devs[0]["T"] and devs[1]["V"] < devs[0]["V"]
    # one set of buffers that holds either mesh: the totals the call is told are the capacities, the offsets say what is there
    V, T, G = devs[0]["V"], devs[0]["T"], 3
    held = {"vertices": torch.zeros((V, 3), device="cuda"), "triangles": torch.zeros((T, 3), dtype=torch.int32, device="cuda"),
            "vertex_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda"), "triangle_offsets": torch.zeros(G + 1, dtype=torch.int32, device="cuda")}

    def load(which):
        dev = devs[which]
        held["vertices"].zero_()
        held["triangles"].zero_()
        held["vertices"][:dev["V"]].copy_(dev["vertices"][:dev["V"]])
        held["triangles"][:dev["T"]].copy_(dev["triangles"][:dev["T"]])
        held["vertex_offsets"].copy_(dev["vertex_offsets"])
        held["triangle_offsets"].copy_(dev["triangle_offsets"])

    wants = []
    for mesh in (large, small):                                         # the reference is told the capacities too: the rows behind are unowned
        padded = plain(mesh)
        padded["vertices"] = np.concatenate([mesh["vertices"], np.zeros((V - len(mesh["vertices"]), 3), F)])
        padded["triangles"] = np.concatenate([mesh["triangles"], np.zeros((T - len(mesh["triangles"]), 3), np.int32)])
        wants.append(sm.smooth(padded, steps=steps))
    load(0)
    out, rows, shapes = allocate(V, T, G, OUTPUTS)
    s = surface.smooth_struct(held["vertices"], held["triangles"], held["vertex_offsets"], held["triangle_offsets"], V, T, out["out_vertices"],
                              out["counts"], steps=steps, **{k: t for k, t in out.items() if k not in ("out_vertices", "counts")})
    lib = _lib.load()
    size = C.c_size_t()
    _lib.check(lib.pr_mesh_smooth_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_smooth_workspace_size")
    workspace = torch.full((size.value // 4 + 64,), POISON, dtype=torch.int32, device="cuda")
    call = lambda: _lib.check(lib.pr_mesh_smooth(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream), "pr_mesh_smooth")
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
    print("recorded smooth:", census)
    assert census == {"nodes": KERNELS + steps, "kernels": KERNELS + steps, "memsets": 0, "memcpys": 0}
    for which in (0, 1, 0):
        load(which)
        for t in out.values():
            t.view(torch.int32).fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        got = {key: t[:rows[key]].reshape(shapes[key]) for key, t in out.items()}
        assert_smooth_equal(got, wants[which], ("replay", which))
        for key, n in rows.items():
            assert bool(is_poison(out[key][n:]).all()), key
        assert bool(is_poison(workspace[size.value // 4:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the consumers
def test_audit_contains_and_distance_on_smoothed_meshes():
    mesh, axes = level_lattice_capped()
    whole = to_meshes(mesh)[0].welded()
    smooth = whole.smoothed(weld=False, iterations=5)
    assert torch.equal(smooth.triangles, whole.triangles) and not torch.equal(smooth.vertices, whole.vertices)
    one, two = whole.audit(), smooth.audit()
    assert torch.equal(one.counts, two.counts) and one.report()["balanced"] and two.report()["balanced"]      # the topology is untouched
    grid = surface.RayGrid.build([smooth], *surface.bounding_grid([smooth], 16))
    points = smooth.vertices[::7] * 0.5
    inside = grid.contains(points)
    assert inside.numel() == points.size(0) and bool(inside.any()) and not bool(inside.all())
    # the noisy sphere comes closer to the clean one
    sphere = wr.weld(ir.pack([ir.part("sphere")[0]]))
    scale = F(1) + np.random.default_rng(0).uniform(-0.05, 0.05, (len(sphere["vertices"]), 1)).astype(F)
    clean = surface.Mesh(cuda(sphere["vertices"]), cuda(sphere["triangles"]))
    noisy = surface.Mesh(cuda((sphere["vertices"] * scale).astype(F)), clean.triangles)
    before = noisy.distance_to(clean, max_distance=0.5)
    after = noisy.smoothed(weld=False).distance_to(clean, max_distance=0.5)
    print("mean distance of the noisy sphere from the clean one:", float(before.mean()), "->", float(after.mean()))
    assert float(after.mean()) < float(before.mean())


# ---------------------------------------------------------------------------------------------------------------------
# 7. the python layer
def test_smooth_meshes_mesh_smoothed_vertex_normals_and_incidence_agree():
    packed = welded("noise", 3)
    vo, to = packed["vertex_offsets"].tolist(), packed["triangle_offsets"].tolist()
    meshes = to_meshes(plain(packed))
    features = [torch.randn(m.vertices.size(0), 5, device="cuda") for m in meshes]
    old_normals = [torch.randn(m.vertices.size(0), 3, device="cuda") for m in meshes]
    for m, f, n in zip(meshes, features, old_normals):
        m.features, m.normals = f, n
    bits = lambda t: t.view(torch.int32)
    for kw, ref in ((dict(), dict(steps=20)), (dict(iterations=3, mu=None, lam=0.25), dict(steps=3, lam=0.25, mu=0.25)),
                    (dict(iterations=2, pin_border=False, max_degree=5), dict(steps=4, flags=0, max_degree=5))):
        want = sm.smooth(plain(packed), **ref)
        out, counts, states = surface.smooth_meshes(meshes, weld=False, report=True, **kw)
        assert len(out) == 3
        for g, m in enumerate(meshes):
            alone, alone_counts, alone_state = m.smoothed(weld=False, report=True, **kw)
            for other in (out[g], alone, m.smoothed(weld=False, **kw)):
                assert torch.equal(bits(other.vertices), bits(cuda(want["vertices"][vo[g]:vo[g + 1]])))
                assert torch.equal(bits(other.normals), bits(cuda(want["normals"][vo[g]:vo[g + 1]])))
                assert other.triangles is m.triangles and other.features is m.features       # carried row for row
            for c, s in ((counts[g], states[g]), (alone_counts, alone_state)):
                assert torch.equal(c, cuda(want["counts"][g])) and torch.equal(s, cuda(want["state"][vo[g]:vo[g + 1]]))
            kept = m.smoothed(weld=False, normals=False, **kw)
            assert kept.normals is m.normals and torch.equal(bits(kept.vertices), bits(out[g].vertices))
    # vertex_normals: the same vertices, normals from the triangles; incidence: the CSR
    want = sm.smooth(plain(packed))
    for g, m in enumerate(meshes):
        fresh = m.vertex_normals()
        assert torch.equal(fresh.vertices, m.vertices) and torch.equal(bits(fresh.normals), bits(cuda(want["normals"][vo[g]:vo[g + 1]])))
        assert fresh.features is m.features
        offsets, triangles = m.incidence()
        start = int(want["incidence_offsets"][vo[g]])
        assert torch.equal(offsets, cuda(want["incidence_offsets"][vo[g]:vo[g + 1] + 1] - start))
        assert triangles.numel() == 3 * (to[g + 1] - to[g])
        assert torch.equal(triangles[:int(offsets[-1])], cuda(want["incidence"][start:start + int(offsets[-1])]))
    # a mask per mesh
    masks = [None, torch.rand(meshes[1].vertices.size(0), device="cuda") < 0.5, None]
    flat = np.zeros(vo[3], np.uint8)
    flat[vo[1]:vo[2]] = masks[1].cpu().numpy()
    want = sm.smooth(plain(packed), pinned=flat, steps=4)
    out = surface.smooth_meshes(meshes, weld=False, iterations=2, pinned=masks)
    for g in range(3):
        assert torch.equal(bits(out[g].vertices), bits(cuda(want["vertices"][vo[g]:vo[g + 1]])))
    with pytest.raises(ValueError, match="one mask"):
        surface.smooth_meshes(meshes, weld=False, pinned=masks[:2])
    with pytest.raises(ValueError, match="one entry per vertex"):
        surface.smooth_meshes(meshes, weld=False, pinned=[None, masks[1][:-1], None])
    # empty meshes
    empty = surface.Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    for weld in (True, False):
        out, counts, state = empty.smoothed(weld=weld, report=True)
        assert out.vertices.shape == (0, 3) and out.normals.shape == (0, 3) and not counts.any() and state.numel() == 0
    offsets, triangles = empty.incidence()
    assert offsets.tolist() == [0] and triangles.numel() == 0


def test_weld_true_is_smoothing_weld_meshes_output_and_features_are_carried():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    field, level = make_field("noise", shape, axes, seed=3)
    unwelded = surface.extract_surface(cuda(field[None]), [cuda(a) for a in axes], level, close_border=True)
    for m in unwelded:
        m.features = torch.randn(m.vertices.size(0), 4, device="cuda")
    first = surface.weld_meshes(unwelded)
    want = surface.smooth_meshes(first, weld=False, iterations=3)
    got = surface.smooth_meshes(unwelded, iterations=3)
    alone = unwelded[0].smoothed(iterations=3)
    for a, b, w in ((got[0], want[0], first[0]), (alone, want[0], first[0])):
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
        assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32)) and torch.equal(a.features, w.features)
        assert a.vertices.size(0) == w.vertices.size(0) < unwelded[0].vertices.size(0)


def test_extract_surface_smooth_is_smooth_meshes_of_the_welded_meshes():
    shape = (9, 17, 33)
    axes = [np.linspace(-1, 1, n).astype(F) for n in shape]
    field, level = make_field("noise", shape, axes, seed=3)
    sigma, device_axes = cuda(field[None]), [cuda(a) for a in axes]
    for kw in ({}, {"simplify": 2, "keep_duplicates": True, "close_border": True}, {"normals": False}):
        today = surface.extract_surface(sigma, device_axes, level, **kw)
        zero = surface.extract_surface(sigma, device_axes, level, smooth=0, **kw)
        for a, b in zip(today, zero):                                   # smooth=0: bit for bit today's result
            assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
            assert (a.normals is None) == (b.normals is None) and (a.normals is None or torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32)))
        got = surface.extract_surface(sigma, device_axes, level, smooth=4, **kw)
        base = surface.extract_surface(sigma, device_axes, level, weld=True, **kw)
        want = surface.smooth_meshes(base, iterations=4, weld=False, normals="normals" not in kw)
        also = surface.extract_surface(sigma, device_axes, level, smooth=4, weld=True, **kw)
        for a, b, c, w in zip(got, want, also, base):
            assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
            assert torch.equal(a.vertices, c.vertices) and not torch.equal(a.vertices, w.vertices)
            assert (a.normals is None) == (b.normals is None) == ("normals" in kw)
            assert a.normals is None or torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    for smooth in (-1, 1.5, None, 2049):
        with pytest.raises(ValueError, match="smooth must be an integer"):
            surface.extract_surface(sigma, device_axes, level, smooth=smooth)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the composer
def test_extract_mesh_smooth_smooths_before_the_feature_query():
    """``extract_mesh(simplify=2, features=True)`` of the small tennis ``player_1`` network at resolution 24, level = the median: with
    ``smooth=3`` the mesh is ``smooth_meshes`` of the welded one in geometry, and its features are those of a ``query_object`` at its
    own - smoothed - vertices."""
    cfg, comp = tennis("fp32")
    style, deformation = codes(cfg)
    with torch.no_grad():
        sigma, _ = comp.density_grid(PLAYER_1, 24, style, deformation)
        level = float(sigma.median())
        kw = dict(level=level, simplify=2, features=True)
        base = comp.extract_mesh(PLAYER_1, 24, style, deformation, weld=True, **kw)
        got = comp.extract_mesh(PLAYER_1, 24, style, deformation, smooth=3, **kw)
        want = surface.smooth_meshes([surface.Mesh(m.vertices, m.triangles, m.normals) for m in base], iterations=3, weld=False)
        G, most = len(got), max(m.vertices.size(0) for m in got)
        points = got[0].vertices[:1].expand(G, most, 3).clone()
        for g, m in enumerate(got):
            points[g, :m.vertices.size(0)] = m.vertices
        features = comp.query_object(PLAYER_1, points, style, deformation)["features"]
    assert len(base) == len(got) == 2 and base[0].triangles.size(0) > 0
    for g, (a, b, w) in enumerate(zip(got, want, base)):
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.triangles, b.triangles)
        assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32)) and not torch.equal(a.vertices, w.vertices)
        assert a.features.shape == w.features.shape and torch.equal(a.features, features[g, :a.vertices.size(0)])
        assert not torch.equal(a.features, w.features)                  # queried at the smoothed vertices, not carried
        print(f"group {g}: V {a.vertices.size(0)}, T {a.triangles.size(0)}")

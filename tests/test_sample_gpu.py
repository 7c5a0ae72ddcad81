"""Surface sampling on the GPU (python -m pytest tests -m gpu): ``pr_mesh_sample`` against its restatement in numpy and Python integers
(tests/sample_reference.py) - points, triangles, barycentrics, normals, attribute rows, counts and measures BIT FOR BIT - through the
C ABI on NaN-poisoned outputs and a NaN-poisoned workspace with guard rows behind every array: triangle counts at the seams of the
blocks and one above 256 x 256, sample counts at the seams of a wave and a block, attribute widths at the seams of the 16-byte
accesses, empty and entirely dropped groups, broken triangles, a triangle too small to be drawn, hostile offsets, the stream index
across 2^32 and windows of a stream, both normal modes, equal bits from call to call, a recorded call replayed, the generator against
``pr_noise_fill``, and the consumers: ``Mesh.sample``, ``RayGrid.sample``, ``closest`` of a mesh's own samples and ``compare_meshes``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib, frame_graph, surface
from playableenvironments_amd.surface import Mesh
from tests import sample_reference as sp

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x7FF80001                # a NaN as fp32, a NaN as fp64 (twice the word), and no triangle index
GUARD = 8                          # rows behind every output that must stay poisoned
SEED = 0x5EED5A3B1E5
OUTPUTS = ("triangle", "barycentric", "out_normals", "out_attributes")
KEYS = {"points": "points", "triangle": "triangle", "barycentric": "barycentric", "out_normals": "normals", "out_attributes": "attributes",
        "counts": "counts", "measures": "measures"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# meshes (numpy only)
def soup(sizes, V=97, C_=4, seed=0):
    """A packed triangle soup: per group ``V`` random vertices and ``sizes[g]`` random triangles with three different indices - areas
    spread over several orders of magnitude -, random (not unit) normals with a zero row, and ``C_`` attribute columns."""
    rng = np.random.default_rng(seed)
    vertices, triangles, vo, to = [], [], [0], [0]
    for T in sizes:
        Vg = V if T else 0
        vertices.append(rng.uniform(-1, 1, (Vg, 3)).astype(F) * F(10.0) ** rng.integers(-2, 1, (Vg, 1)).astype(F))
        t = np.stack([rng.permutation(Vg)[:3] for _ in range(min(T, 512))]).reshape(-1, 3) if T else np.zeros((0, 3), np.int64)
        if T > len(t):                                              # (large groups: shifted copies of distinct triples stay distinct)
            more = rng.integers(0, Vg, (T - len(t), 1))
            t = np.concatenate([t, (t[rng.integers(0, len(t), T - len(t))] + more) % Vg])
        triangles.append(t.astype(np.int32))
        vo.append(vo[-1] + Vg)
        to.append(to[-1] + T)
    mesh = {"vertices": np.concatenate(vertices).reshape(-1, 3), "triangles": np.concatenate(triangles).reshape(-1, 3).astype(np.int32),
            "vertex_offsets": np.array(vo, np.int32), "triangle_offsets": np.array(to, np.int32)}
    rows = len(mesh["vertices"])
    mesh["normals"] = rng.normal(size=(rows, 3)).astype(F)
    if rows:
        mesh["normals"][rows // 2] = 0
    mesh["attributes"] = rng.normal(size=(rows, C_)).astype(F)
    return mesh


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device(mesh):
    """The packed input as device tensors (at least one row each: an empty tensor has no address)."""
    pad = lambda a: cuda(a if len(a) else np.zeros((1,) + a.shape[1:], dtype=a.dtype))
    out = {k: pad(mesh[k]) for k in ("vertices", "triangles", "normals", "attributes") if mesh.get(k) is not None}
    out["vertex_offsets"], out["triangle_offsets"] = cuda(np.asarray(mesh["vertex_offsets"], np.int32)), cuda(np.asarray(mesh["triangle_offsets"], np.int32))
    out["V"], out["T"] = int(mesh.get("V", len(mesh["vertices"]))), int(mesh.get("T", len(mesh["triangles"])))
    return out


def poisoned(words):
    return torch.full((words,), POISON, dtype=torch.int32, device="cuda")


def is_poison(t):
    return t.view(torch.int32) == POISON


def allocate(G, n, C_, outputs):
    """Poisoned outputs with guard rows, as int32 words: ``(buffers, words, views)``."""
    shapes = {"points": ((G, n, 3), torch.float32), "counts": ((G, 4), torch.int32), "measures": ((G, 2), torch.float64)}
    if "triangle" in outputs:
        shapes["triangle"] = ((G, n), torch.int32)
    if "barycentric" in outputs:
        shapes["barycentric"] = ((G, n, 2), torch.float32)
    if "out_normals" in outputs:
        shapes["out_normals"] = ((G, n, 3), torch.float32)
    if "out_attributes" in outputs:
        shapes["out_attributes"] = ((G, n, C_), torch.float32)
    buffers, words = {}, {}
    for key, (shape, dtype) in shapes.items():
        words[key] = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
        buffers[key] = poisoned(words[key] + 4 * GUARD)
    return buffers, words, shapes


def describe(dev, n, seed, buffers, first=0, face=False, attributes=True):
    """``pr_mesh_sample_t`` over the device mesh and the poisoned buffers (the optional outputs are those that ``buffers`` holds)."""
    view = lambda key, dtype: None if key not in buffers else buffers[key].view(dtype)
    return surface.sample_struct(dev["vertices"], dev["triangles"], dev["vertex_offsets"], dev["triangle_offsets"], dev["V"], dev["T"], n, seed,
                                 view("points", torch.float32), view("counts", torch.int32), view("measures", torch.float64), first=first,
                                 face_normals=face, normals=None if face else dev["normals"],
                                 attributes=dev["attributes"] if attributes else None, triangle=view("triangle", torch.int32),
                                 barycentric=view("barycentric", torch.float32), out_normals=view("out_normals", torch.float32),
                                 out_attributes=view("out_attributes", torch.float32))


def run_sample(dev, n, seed=SEED, first=0, face=False, outputs=OUTPUTS):
    """One call on poisoned outputs and a poisoned workspace, guard words behind every array.  Returns the outputs without their
    guards (which are checked here)."""
    G = dev["vertex_offsets"].numel() - 1
    C_ = dev["attributes"].size(1)
    buffers, words, shapes = allocate(G, n, C_, outputs)
    s = describe(dev, n, seed, buffers, first=first, face=face, attributes="out_attributes" in outputs)
    lib, size = _lib.load(), C.c_size_t()
    _lib.check(lib.pr_mesh_sample_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_sample_workspace_size")
    workspace = poisoned(size.value // 4 + 64)                         # (64 guard words)
    _lib.check(lib.pr_mesh_sample(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream), "pr_mesh_sample")
    torch.cuda.synchronize()
    assert bool(is_poison(workspace[size.value // 4:]).all()), "workspace guard"
    for key, t in buffers.items():
        assert bool(is_poison(t[words[key]:]).all()), ("guard", key)
    return {key: t[:words[key]].view(shapes[key][1]).reshape(shapes[key][0]) for key, t in buffers.items()}


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def assert_sample_equal(got, want, what):
    """Every output on its words (floats as bits: the sign of zero counts)."""
    for key, t in got.items():
        expected = cuda(want[KEYS[key]])
        assert expected.shape == t.shape and expected.dtype == t.dtype, (what, key, expected.shape, t.shape, expected.dtype, t.dtype)
        wrong = bits(t) != bits(expected)
        assert not bool(wrong.any()), (what, key, int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())


def reference(mesh, n, seed=SEED, first=0, face=False, outputs=OUTPUTS):
    return sp.sample(mesh, n, seed, first, normals=mesh["normals"] if "out_normals" in outputs and not face else None,
                     attributes=mesh["attributes"] if "out_attributes" in outputs else None, face=face and "out_normals" in outputs)


def check_case(mesh, n, what, again=True, **kw):
    """The call with every output against the reference, and a second call into fresh buffers against the first."""
    want = reference(mesh, n, **kw)
    dev = device(mesh)
    got = run_sample(dev, n, **kw)
    assert_sample_equal(got, want, what)
    if again:
        second = run_sample(dev, n, **kw)
        for key in got:
            assert torch.equal(bits(got[key]), bits(second[key])), (what, key, "second call")
    return got, want


# ---------------------------------------------------------------------------------------------------------------------
# 1. the seams
@pytest.mark.parametrize("T", [1, 255, 256, 257, 65537])
def test_triangle_counts_at_the_seams_of_the_blocks_and_of_the_block_sum_scan(T):
    """65 537 triangles are 257 blocks: the scan of the block sums crosses its own chunk of 256."""
    mesh = soup([T, 3], seed=T)
    got, want = check_case(mesh, 257, ("T", T))
    assert got["counts"][:, 0].tolist() == [T, 3] and got["counts"][:, 3].tolist() == [257, 257]
    drawn = torch.unique(got["triangle"][0])
    assert int(drawn.min()) >= 0 and int(drawn.max()) < T
    if T == 65537:
        assert int(got["triangle"][0].max()) >= 65536 - 4096, "the last blocks are reachable"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sample_counts_at_the_seams_of_a_wave_and_a_block(n):
    got, _ = check_case(soup([257, 40], seed=1), n, ("n", n))
    assert got["points"].shape == (2, n, 3) and got["counts"][:, 3].tolist() == [n, n]


@pytest.mark.parametrize("C_", [1, 3, 4, 191, 192, 193])
def test_attribute_widths_at_the_seams_of_the_vector_accesses(C_):
    got, _ = check_case(soup([300, 7], C_=C_, seed=C_), 65, ("C", C_))
    assert got["out_attributes"].shape == (2, 65, C_) and bool(torch.isfinite(got["out_attributes"]).all())


def test_rows_that_are_not_16_byte_aligned_take_the_scalar_path():
    """C = 192 with the attribute rows one word off a 16-byte boundary: the same bits as the aligned call."""
    mesh = soup([300], C_=192, seed=5)
    dev = device(mesh)
    want = run_sample(dev, 65)
    shifted = torch.empty(dev["attributes"].numel() + 4, dtype=torch.float32, device="cuda")
    shifted[1:1 + dev["attributes"].numel()] = dev["attributes"].reshape(-1)
    off = dict(dev, attributes=shifted[1:1 + dev["attributes"].numel()].view(-1, 192))
    assert off["attributes"].data_ptr() % 16 == 4
    got = run_sample(off, 65)
    for key in want:
        assert torch.equal(bits(got[key]), bits(want[key])), key


# ---------------------------------------------------------------------------------------------------------------------
# 2. empty, dropped, broken and tiny
def broken(mesh, seed=2):
    """A copy with degenerate (collinear), out-of-range, repeated-index and NaN / inf triangles mixed in."""
    rng = np.random.default_rng(seed)
    out = {k: v.copy() for k, v in mesh.items()}
    vo, to = out["vertex_offsets"], out["triangle_offsets"]
    for g in range(len(to) - 1):
        rows = np.arange(to[g], to[g + 1])
        if not len(rows):
            continue
        Vg = vo[g + 1] - vo[g]
        pick = rng.uniform(0, 1, len(rows))
        out["triangles"][rows[pick < 0.05], 1] = -1
        out["triangles"][rows[(pick >= 0.05) & (pick < 0.1)], 2] = Vg
        out["triangles"][rows[(pick >= 0.1) & (pick < 0.12)], 0] = 2 ** 31 - 1
        same = rows[(pick >= 0.12) & (pick < 0.2)]
        out["triangles"][same, 2] = out["triangles"][same, 0]
        out["vertices"][vo[g] + 1] = [np.nan, 0, 0]
        out["vertices"][vo[g] + 2] = [0, np.inf, 0]
        out["vertices"][vo[g] + 3] = 2 * out["vertices"][vo[g] + 4] - out["vertices"][vo[g] + 5]        # (collinear with 4 and 5, nearly)
        out["vertices"][vo[g] + 6] = out["vertices"][vo[g] + 7]                                        # (equal as values, not as indices)
    return out


def test_three_groups_with_an_empty_middle_group_and_a_group_that_is_all_dropped():
    mesh = broken(soup([300, 0, 200, 50], seed=3))
    to = mesh["triangle_offsets"]
    mesh["triangles"][to[3]:to[4], 1] = mesh["triangles"][to[3]:to[4], 0]          # group 3: every triangle repeats an index
    for face in (False, True):
        got, want = check_case(mesh, 65, ("empty", face), face=face)
        counts = got["counts"].tolist()
        assert counts[1] == [0, 0, 0, 0] and counts[3] == [0, 50, 0, 0] and counts[0][1] > 0 and counts[0][0] > 0 and counts[0][3] == 65
        for g in (1, 3):
            assert bool((got["triangle"][g] == -1).all()) and not got["measures"][g].any()
            for key in ("points", "barycentric", "out_normals", "out_attributes"):
                assert not bits(got[key][g]).any(), (key, g)
        # no dropped triangle is ever drawn
        for g in (0, 2):
            w = np.array(want["groups"][g]["w"], dtype=np.float64)
            assert (w[got["triangle"][g].cpu().numpy()] > 0).all()


def test_a_triangle_2_to_the_minus_40_of_the_largest_has_weight_0_and_is_never_drawn():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [2 + 2.0 ** -20, 2, 2], [2, 2 + 2.0 ** -20, 2], [0, 0, 1]], F)
    t = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 6]], np.int32)
    mesh = {"vertices": v, "triangles": t, "vertex_offsets": np.array([0, 7], np.int32), "triangle_offsets": np.array([0, 3], np.int32),
            "normals": np.ones((7, 3), F), "attributes": np.arange(28, dtype=F).reshape(7, 4)}
    got, want = check_case(mesh, 257, "tiny")
    assert want["groups"][0]["area"][0] == 2.0 ** -41 and want["groups"][0]["w"] == [0, 2 ** 32, 2 ** 32]
    assert got["counts"].tolist() == [[3, 0, 1, 257]] and not bool((got["triangle"] == 0).any())
    assert got["measures"].tolist() == [[0.5, 1.0]]


def test_hostile_offsets_are_clamped_and_cost_their_own_group_at_most():
    base = broken(soup([300, 200, 100], seed=4))
    vo, to = base["vertex_offsets"].tolist(), base["triangle_offsets"].tolist()
    V, T = vo[-1], to[-1]
    clean = check_case(base, 65, "values", again=False)[0]
    for name, v_off, t_off in (("decreasing", [0, vo[2], vo[1], V], [0, to[2], to[1], T]),
                               ("leaving", [-5, vo[1], V + 1000, 2 ** 31 - 1], [-2 ** 31, to[1], T + 7, T + 9]),
                               ("late", [7, vo[1], vo[2], V - 3], [11, to[1], to[2], T - 5])):
        changed = dict(base, vertex_offsets=np.array(v_off, np.int32), triangle_offsets=np.array(t_off, np.int32))
        got, _ = check_case(changed, 65, name, again=False)
        if name == "leaving":                                          # group 0 is as it was: its rows are those of the clean call
            for key in got:
                assert torch.equal(bits(got[key][0]), bits(clean[key][0])), (name, key)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the stream
def test_the_stream_index_carries_into_the_second_counter_word_and_windows_of_a_stream_agree():
    mesh = soup([257, 40], seed=6)
    dev = device(mesh)
    first = 2 ** 32 - 3
    got, _ = check_case(mesh, 65, "carry", first=first)
    for k in (1, 3, 4, 64):
        window = run_sample(dev, 65 - k, first=first + k)
        for key in ("points", "triangle", "barycentric", "out_normals", "out_attributes"):
            assert torch.equal(bits(window[key]), bits(got[key][:, k:])), (k, key)
    check_case(mesh, 5, "wrap", first=2 ** 64 - 2, again=False)
    other = run_sample(dev, 65, first=first + 65)
    assert not bool((bits(other["barycentric"]) == bits(got["barycentric"])).all(dim=2).any()), "disjoint ranges, disjoint draws"
    seeded = run_sample(dev, 65, seed=SEED + 1, first=first)
    assert not torch.equal(seeded["triangle"], got["triangle"])


def test_optional_outputs_and_both_normal_modes():
    mesh = soup([300, 40], seed=7)
    full = {face: check_case(mesh, 65, ("all", face), face=face)[0] for face in (False, True)}
    assert not torch.equal(bits(full[False]["out_normals"]), bits(full[True]["out_normals"]))
    length = full[True]["out_normals"].double().norm(dim=2)
    assert bool(((length - 1).abs() < 1e-6).all())
    for outputs in ((), ("triangle",), ("barycentric", "out_attributes"), ("out_normals",)):
        for face in (False, True):
            got, _ = check_case(mesh, 65, (outputs, face), again=False, face=face, outputs=outputs)
            for key in got:
                assert torch.equal(bits(got[key]), bits(full[face][key])), (outputs, key)


def _noise_fill(seed, kind, ty, obj, shape):
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().pr_noise_fill(C.c_uint64(seed), kind, ty, obj, out.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "pr_noise_fill")
    return out


def test_the_restated_generator_is_the_devices():
    """``pr_noise_fill`` draws from philox4x32_10 with the counter (index, 0, 0) and the key mix(seed ^ salt): its uniform stream is
    ``(x[0] >> 8) 2^-24`` exactly, its normal stream Box-Muller of x[0] and x[1].  (x[2] and x[3] are not reachable through it:
    the known-answer vectors of test_sample_cpu.py and the barycentrics above, bit for bit, hold them.)"""
    seed, n = 1234, 4096
    salt = lambda kind, ty, obj: sp.noise_mix(kind * 16 + ty * 8 + obj + 1)
    index = np.arange(n, dtype=np.uint64)
    key = sp.noise_mix(seed ^ salt(0, 0, 0))
    x = sp.philox4x32_10(index, 0, 0, 0, key & sp.M32, key >> 32)
    uniform = (x[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    assert np.array_equal(_noise_fill(seed, 0, 0, 0, (n,)).cpu().numpy().astype(np.float64), uniform)
    key = sp.noise_mix(seed ^ salt(3, 0, 2))
    x = sp.philox4x32_10(index, 0, 0, 0, key & sp.M32, key >> 32)
    u1 = ((x[0] >> np.uint64(8)).astype(np.float64) + 1) * 2.0 ** -24
    u2 = (x[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    normal = np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    assert np.abs(_noise_fill(seed, 3, 0, 2, (n,)).cpu().numpy() - normal).max() < 1e-4      # (fp32 log, cos and sqrt of values below 6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a recorded call
def test_recorded_call_holds_kernels_only_and_replays_with_equal_bits():
    mesh = soup([300, 0, 700], C_=192, seed=8)
    dev = device(mesh)
    n, G = 257, 3
    want = reference(mesh, n)
    for outputs, kernels in ((OUTPUTS, 8), (("triangle", "out_normals"), 7)):
        buffers, words, shapes = allocate(G, n, 192, outputs)
        s = describe(dev, n, SEED, buffers, attributes="out_attributes" in outputs)
        lib, size = _lib.load(), C.c_size_t()
        _lib.check(lib.pr_mesh_sample_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_sample_workspace_size")
        workspace = poisoned(size.value // 4 + 64)
        call = lambda: _lib.check(lib.pr_mesh_sample(C.byref(s), workspace.data_ptr(), size.value, torch.cuda.current_stream().cuda_stream),
                                  "pr_mesh_sample")
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
        print("recorded sample:", census)
        assert census == {"nodes": kernels, "kernels": kernels, "memsets": 0, "memcpys": 0}
        for _ in range(2):
            for t in buffers.values():
                t.fill_(POISON)
            workspace.fill_(POISON)
            graph.replay()
            torch.cuda.synchronize()
            got = {key: t[:words[key]].view(shapes[key][1]).reshape(shapes[key][0]) for key, t in buffers.items()}
            assert_sample_equal(got, want, ("replay", outputs))
            for key, t in buffers.items():
                assert bool(is_poison(t[words[key]:]).all()), key
            assert bool(is_poison(workspace[size.value // 4:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. the consumers
def icosphere(level=4, radius=1.0):
    """A sphere mesh with every vertex at ``radius`` from the origin (fp32 rounding apart): ``(vertices fp32, triangles int32)``."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        middle, new = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                middle[key] = len(v) - 1
            return middle[key]
        for a, b, c in t:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            new += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = new
    return (np.array(v) * radius).astype(F), np.array(t, dtype=np.int32)


_SPHERE = {}


def sphere_meshes():
    if not _SPHERE:
        v, t = icosphere()
        _SPHERE["a"] = Mesh(cuda(v), cuda(t))
        _SPHERE["b"] = Mesh(cuda(v) * 1.01, cuda(t))
    return _SPHERE["a"], _SPHERE["b"]


def test_mesh_sample_and_ray_grid_sample_agree_with_sample_meshes():
    mesh = soup([300, 40], C_=192, seed=9)
    vo, to = mesh["vertex_offsets"], mesh["triangle_offsets"]
    meshes = [Mesh(cuda(mesh["vertices"][vo[g]:vo[g + 1]]), cuda(mesh["triangles"][to[g]:to[g + 1]]), cuda(mesh["normals"][vo[g]:vo[g + 1]]),
                   cuda(mesh["attributes"][vo[g]:vo[g + 1]]).to(torch.float16 if g else torch.float32)) for g in range(2)]
    half = dict(mesh, attributes=np.concatenate([mesh["attributes"][:vo[1]], mesh["attributes"][vo[1]:].astype(np.float16).astype(F)]))
    want = sp.sample(half, 65, SEED, 5, normals=mesh["normals"], attributes=half["attributes"])
    got = surface.sample_meshes(meshes, 65, seed=SEED, first=5, normals="vertex")
    names = (("points", "points"), ("triangle", "triangle"), ("barycentric", "barycentric"), ("normals", "normals"), ("features", "attributes"),
             ("counts", "counts"), ("measures", "measures"))
    for g in range(2):
        for mine, theirs in names:
            assert torch.equal(bits(getattr(got[g], mine)), bits(cuda(want[theirs][g]))), (g, mine)
    # one mesh alone is group 0 of its own call
    alone = meshes[0].sample(65, seed=SEED, first=5, normals="vertex")
    for mine, _ in names:
        assert torch.equal(bits(getattr(alone, mine)), bits(getattr(got[0], mine))), mine
    assert meshes[0].sample(9, seed=1, normals=None, features=False).normals is None
    assert meshes[0].sample(9, seed=1, features=False).features is None
    # the grid samples the packed arrays it holds: face normals
    grid = surface.RayGrid.build(meshes, *surface.bounding_grid(meshes, 8))
    faces = surface.sample_meshes(meshes, 65, seed=SEED, first=5, normals="face", features=False)
    for g, s in enumerate(grid.sample(65, seed=SEED, first=5)):
        for mine in ("points", "triangle", "barycentric", "normals", "counts", "measures"):
            assert torch.equal(bits(getattr(s, mine)), bits(getattr(faces[g], mine))), (g, mine)
        assert s.features is None
    with pytest.raises(ValueError, match="holds no vertex normals"):
        grid.sample(4, seed=1, normals="vertex")
    with pytest.raises(ValueError, match="needs meshes with normals"):
        Mesh(meshes[0].vertices, meshes[0].triangles).sample(4, seed=1, normals="vertex")


def test_closest_finds_a_meshs_own_samples_on_it():
    """The point is ((b0 a) + (b1 b)) + (b2 c) in fp32: three products and two sums, each within 2^-24 relative of a value that a
    convex combination keeps at or below M, the largest |coordinate|: at most 5 * 2^-24 M per component, sqrt(3) times that as a
    distance, 0.54 * 2^-20 M, from the exact point of the triangle.  The query's own fp32 evaluation of a distance this small has the
    same size.  2^-20 M holds both."""
    a, _ = sphere_meshes()
    samples = a.sample(4096, seed=SEED)
    grid = surface.RayGrid.build([a], *surface.bounding_grid([a], 32))
    found = grid.closest(samples.points, max_distance=0.05, barycentric=True)
    bound = 2.0 ** -20 * float(a.vertices.abs().max())
    print("largest distance of a sample from its own mesh:", float(found.distance.max()), "bound", bound)
    assert bool((found.triangle >= 0).all()) and float(found.distance.max()) <= bound


def test_compare_meshes_of_a_mesh_with_itself_and_of_a_sphere_with_the_sphere_scaled_by_1_01():
    a, b = sphere_meshes()
    same = surface.compare_meshes(a, a, samples=4096, seed=SEED, max_distance=0.05, thresholds=(0.001,)).report()
    # (normal consistency: a sample within rounding of an edge may find the neighbouring triangle, whose normal is a few degrees off)
    for side in ("a_to_b", "b_to_a"):
        assert same[side]["misses"] == 0 and same[side]["samples"] == 4096 and same[side]["max"] <= 2.0 ** -20 * 1.0
        assert same[side]["within"] == [1.0] and same[side]["normal_consistency"] > 1 - 1e-4
    assert same["thresholds"][0]["fscore"] == 1.0
    # The chord error: every point p of a has r_min <= |p| <= 1, r_min the distance of the closest face plane from the origin, and
    # every point q of b has |q| >= 1.01 r_min: |q - p| >= 1.01 r_min - |p| >= 1.01 r_min - 1.  And 1.01 p lies on b: the distance
    # is at most 0.01 |p| <= 0.01.  Both with 2^-20 for the fp32 rounding of b's vertices, of the points and of the query.
    v, t = a.vertices.double().cpu().numpy(), a.triangles.cpu().numpy()
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    normal = np.cross(p1 - p0, p2 - p0)
    r_min = float((np.abs((normal * p0).sum(axis=1)) / np.linalg.norm(normal, axis=1)).min())
    low, high = 1.01 * r_min - 1.0 - 2.0 ** -20, 0.01 + 2.0 ** -20
    assert 0.008 < low < high
    deviation = surface.compare_meshes(a, b, samples=4096, seed=SEED, max_distance=0.05, thresholds=(0.005, 0.02))
    report = deviation.report()
    print("sphere against 1.01 sphere:", report, "bounds", low, high)
    assert report["a_to_b"]["misses"] == 0 and report["b_to_a"]["misses"] == 0
    assert low <= report["a_to_b"]["mean"] <= high and low <= report["a_to_b"]["max"] <= high
    assert report["a_to_b"]["within"] == [0.0, 1.0] and report["thresholds"][1]["fscore"] == 1.0 and report["thresholds"][0]["fscore"] == 0.0
    assert report["a_to_b"]["normal_consistency"] > 0.999
    # the reductions against numpy fp64 over the same distances: 1e-9 relative (N * 2^-53 with room)
    for side, distance in (("a_to_b", deviation.distance_a_to_b), ("b_to_a", deviation.distance_b_to_a)):
        d = distance.cpu().numpy().astype(np.float64)
        d = d[np.isfinite(d)]
        ordered = np.sort(d)
        want = {"mean": d.mean(), "rms": math.sqrt((d * d).mean()), "max": d.max(), "p99": ordered[math.ceil(0.99 * len(d)) - 1]}
        for key, value in want.items():
            assert abs(report[side][key] - value) <= 1e-9 * abs(value), (side, key, report[side][key], value)
    assert abs(report["chamfer"] - (report["a_to_b"]["mean"] + report["b_to_a"]["mean"])) == 0
    # beyond max_distance everything is a miss: reported, left out of the means
    far = surface.compare_meshes(a, b, samples=256, seed=SEED, max_distance=0.001, thresholds=(0.001,)).report()
    assert far["a_to_b"]["misses"] == 256 and math.isnan(far["a_to_b"]["mean"]) and far["a_to_b"]["within"] == [0.0]
    assert far["thresholds"][0]["fscore"] == 0.0

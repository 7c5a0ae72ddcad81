"""Host-side checks of retained per-sample state (``pr_render_forward_retained``): the C surface, the cache size against the sum
DESIGN.md section 14 states, the refusals that precede any device work and the host logic of ``retention.Retained``.  No GPU needed."""
import copy
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import warnings

import pytest
import torch

from playableenvironments_amd import ObjectComposer, _lib, configs, retention
from tests.test_occupancy_cpu import _host_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCC_WORDS = 8192        # occupancy key capacity per frame and level


def _a(n):
    return (n + 255) // 256 * 256


def _design_sum(call, objs, mask, defer):
    """The cache size as DESIGN.md 14 states it: every region rounded up to 256 bytes."""
    N, R = call.frames, call.rays
    total = 256 + _a(4 * N * 3) + _a(4 * N * R * 3)
    for k in range(call.objects):
        if not (mask >> k) & 1:
            continue
        levels = [objs[k].coarse] + ([objs[k].fine] if call.use_fine else [])
        total += _a(4 * N * 12) + _a(4 * N) + _a(4 * N * levels[0].style_features) + _a(4 * N * levels[0].deformation_features)
        for m in levels:
            W = m.layers_width
            total += 2 * _a(4 * W) + 2 * _a(4 * (W // 2))
            if m.kind != 1:
                total += _a(4 * N * OCC_WORDS)
        for m in levels:
            cap = N * R * m.positions
            row = (m.layers_width // 2 + 1 + 3) // 4 * 4 if defer else m.output_features
            total += 3 * _a(4 * cap) + (_a(4 * cap) if m.has_bender else 0) + _a(4 * cap * row)
    return total


def _size(lib, call, objs, mask):
    size = C.c_size_t()
    st = lib.pr_retained_size(C.byref(call), objs, mask, C.byref(size))
    return st, size.value


def test_header_declares_the_entry_points_and_the_abi_stays(built_library):
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(pr_\w+)\s*\(", header, flags=re.M))
    assert {"pr_retained_size", "pr_retained_reset", "pr_render_forward_retained"} <= declared
    assert declared == set(_lib.SYMBOLS)
    assert re.search(r"#define PR_ABI_VERSION 5\b", header) and built_library.pr_abi_version() == 5
    assert "typedef struct pr_retained_t" in header
    assert C.sizeof(_lib.Retained) == 40 and _lib.Retained.cache.offset == 16 and _lib.Retained.reused.offset == 32
    # no new preprocessor conditional in the new translation unit
    source = open(os.path.join(ROOT, "playableenvironments_amd", "csrc", "retain.hip")).read()
    assert not re.search(r"^\s*#\s*if", source, flags=re.M)


@pytest.mark.parametrize("case", ["tennis", "tennis_hierarchical", "minecraft"])
def test_retained_size_equals_the_design_sum(built_library, case):
    lib = built_library
    cfg = {"tennis": configs.tennis_config, "minecraft": configs.minecraft_config,
           "tennis_hierarchical": lambda: configs.tennis_config(hierarchical=(16, 32))}[case]()
    comp = ObjectComposer(cfg)
    K = comp.object_id_helper.objects_count
    call, objs = _host_call(comp, K, use_fine=case == "tennis_hierarchical")
    call.frames, call.rays = 2, 529
    static = comp.object_id_helper.static_objects_count
    mask = (1 << static) - 1
    for flags, defer in ((0, False), (_lib.PR_FLAG_DEFER_PROJECTION, True)):
        call.flags = flags
        st, size = _size(lib, call, objs, mask)
        assert st == 0 and size == _design_sum(call, objs, mask, defer) and size % 256 == 0, (case, flags, size)
        st, one = _size(lib, call, objs, 1)
        assert st == 0 and one == _design_sum(call, objs, 1, defer) and one % 256 == 0
        assert one < size or static == 1
        st, none = _size(lib, call, objs, 0)
        assert st == 0 and none == 256 + _a(4 * 2 * 3) + _a(4 * 2 * 529 * 3) and none < one
        st, everything = _size(lib, call, objs, (1 << K) - 1)
        assert st == 0 and everything > size and everything % 256 == 0
    # f16x3 never defers: full-width rows
    call.flags, call.precision = _lib.PR_FLAG_DEFER_PROJECTION, _lib.PR_PRECISION_F16X3
    assert _size(lib, call, objs, mask)[1] == _design_sum(call, objs, mask, False)
    st, _ = _size(lib, call, objs, 1 << K)
    assert st == -1 and b"beyond" in lib.pr_last_error()


def test_retained_entry_point_refuses_what_the_issue_lists_before_any_device_work(built_library):
    lib = built_library
    comp = ObjectComposer(configs.minecraft_config())
    K = comp.object_id_helper.objects_count
    call, objs = _host_call(comp, K)
    outs = _lib.Outputs()
    st, need = _size(lib, call, objs, 0b11)
    assert st == 0

    def retained(mask=0b11, cache=256, size=need):
        r = _lib.Retained()
        r.object_mask, r.cache, r.cache_bytes = mask, cache, size
        return r

    def status(r, workspace=256, size=0, occ=None):
        st = lib.pr_render_forward_retained(C.byref(call), objs, occ, None if r is None else C.byref(r), C.byref(outs), None, workspace,
                                            size, None)
        return st, lib.pr_last_error()

    # a well-formed request passes every host check and stops at the (zero-sized) workspace, before any device work; so does NULL
    for r in (retained(), None, retained(mask=0, size=256 + 256 + _a(4 * 64 * 3))):
        st, msg = status(r)
        assert st == -2 and b"workspace too small" in msg, (st, msg)
    for flag, word in ((_lib.PR_FLAG_PERTURB, b"PR_FLAG_PERTURB"), (_lib.PR_FLAG_TRAIN_BN, b"PR_FLAG_TRAIN_BN"),
                       (_lib.PR_FLAG_SAVE_FOR_BACKWARD, b"PR_FLAG_SAVE_FOR_BACKWARD"), (_lib.PR_FLAG_NAIVE_MLP, b"PR_FLAG_NAIVE_MLP")):
        call.flags = flag
        st, msg = status(retained())
        assert st == -1 and word in msg and b"retention" in msg, (flag, st, msg)
        st, msg = status(None)                    # without retention the flag is the caller's business
        assert b"retention" not in msg
    call.flags = _lib.PR_FLAG_GATE_HEAD | _lib.PR_FLAG_FIX_OVERLAPS | _lib.PR_FLAG_CANONICAL_POSE | _lib.PR_FLAG_DEFER_PROJECTION
    assert status(retained(size=1 << 40))[0] == -2
    call.flags = 0
    for where in ("coarse", "fine"):
        noise = getattr(call, "noise_" + where)
        noise.integrate[1] = 256
        st, msg = status(retained())
        assert st == -1 and b"integrate-noise" in msg
        noise.integrate[1] = None
        noise.integrate_global = 256
        st, msg = status(retained())
        assert st == -1 and b"integrate-noise" in msg
        noise.integrate_global = None
    st, msg = status(retained(mask=1 << K))
    assert st == -1 and b"beyond" in msg
    st, msg = status(retained(cache=128))
    assert st == -1 and b"aligned" in msg
    st, msg = status(retained(cache=None))
    assert st == -1 and b"aligned" in msg
    st, msg = status(retained(size=need - 1))
    assert st == -1 and b"too small" in msg and str(need).encode() in msg
    # a grid on a retained object may have at most 64^3 cells (the cache keeps a copy of its bits)
    def grid(cells, k=0):
        occ = _lib.Occupancy()
        occ.coarse[k].bits = 256
        for a in range(3):
            occ.coarse[k].cells[a] = cells[a]
        occ.coarse[k].words = (cells[0] * cells[1] * cells[2] + 31) // 32
        return occ
    st, msg = status(retained(), occ=C.byref(grid((65, 64, 64))))
    assert st == -1 and b"object 0 is retained" in msg and b"262144" in msg, (st, msg)
    assert status(retained(size=1 << 40), occ=C.byref(grid((64, 64, 64))))[0] == -2
    assert status(retained(mask=0b10, size=1 << 40), occ=C.byref(grid((65, 64, 64))))[0] == -2      # (object 0 is not retained)
    assert status(None, occ=C.byref(grid((65, 64, 64))))[0] == -2
    outs.sample_delta[1] = 256
    st, msg = status(retained())
    assert st == -1 and b"sample_delta" in msg
    assert status(retained(mask=0b01))[0] == -2           # (the export of an object that is not retained is fine)
    outs.sample_delta[1] = None
    assert status(retained())[0] == -2
    # the reset refuses bad caches without a launch
    assert lib.pr_retained_reset(None, 4096, None) == -1 and b"aligned" in lib.pr_last_error()
    assert lib.pr_retained_reset(128, 4096, None) == -1
    assert lib.pr_retained_reset(256, 128, None) == -1 and b"too small" in lib.pr_last_error()


def test_plain_c_client_links_the_three_symbols(built_library, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    source = tmp_path / "client.c"
    source.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "playrender.h"
int main(void) {
    pr_retained_t r;
    size_t bytes = 0;
    memset(&r, 0, sizeof r);
    r.object_mask = 3u;
    if (pr_abi_version() != PR_ABI_VERSION) return 1;
    if (pr_retained_size(NULL, NULL, r.object_mask, &bytes) != PR_ERR_INVALID) return 2;
    if (pr_retained_reset(NULL, 0, NULL) != PR_ERR_INVALID) return 3;
    if (pr_render_forward_retained(NULL, NULL, NULL, &r, NULL, NULL, NULL, 0, NULL) != PR_ERR_INVALID) return 4;
    printf("retained %u %u\n", (unsigned)sizeof r, (unsigned)r.object_mask);
    return 0;
}
""")
    lib_dir = os.path.dirname(_lib.library_path())
    binary = tmp_path / "client"
    build = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(source),
                            "-L", lib_dir, "-lplayrender", f"-Wl,-rpath,{lib_dir}", "-o", str(binary)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "retained 40 3" in run.stdout, (run.returncode, run.stdout, run.stderr[-2000:])


def test_retained_host_logic():
    comp = ObjectComposer(configs.minecraft_config()).eval()
    helper = comp.object_id_helper
    K, static = helper.objects_count, helper.static_objects_count
    assert comp.retained is None
    r = comp.retain_objects()
    assert isinstance(r, retention.Retained) and r.objects == tuple(range(static)) and r.mask == (1 << static) - 1
    assert r.bytes == 0 and r.last_reused is None and r.host_key == 0
    everything = comp.retain_objects(range(K))                     # any object may be named, the skybox included
    assert everything.objects == tuple(range(K)) and everything.signature() != r.signature()
    assert comp.retain_objects([1, 1, 0]).objects == (0, 1)
    with pytest.raises(ValueError, match="out of range"):
        comp.retain_objects([K])
    with pytest.raises(ValueError, match="at least one"):
        comp.retain_objects([])
    # eligibility: the calls the occupancy grid is used on
    comp.retained = r
    with torch.no_grad():
        assert comp._retention_for_call(False, False, None) is r
        assert comp._retention_for_call(True, False, None) is None
        assert comp._retention_for_call(False, True, None) is None
        assert comp._retention_for_call(False, False, [0]) is None
        comp.train()
        assert comp._retention_for_call(False, False, None) is None
        comp.eval()
        comp.use_naive_mlp = True
        assert comp._retention_for_call(False, False, None) is None
        comp.use_naive_mlp = False
        comp.retained = "cache"
        with pytest.raises(TypeError):
            comp._retention_for_call(False, False, None)
        comp.retained = r
    assert comp._retention_for_call(False, False, None) is None          # gradients enabled
    assert "forward_expected_positions" not in inspect.getsource(ObjectComposer._retention_for_call)
    # host_key: the epoch of the weight values, derived from what THIS call's packed weights were made from - it moves when a
    # retained object's model changed since the previous call that used r, also while r was detached, and only then
    model0 = comp.object_models_coarse[helper.model_idx_by_object_idx(0)]
    dynamic = comp.object_models_coarse[helper.model_idx_by_object_idx(K - 1)]

    def use():
        r.weights_seen(comp._retained_weights_key(r))
        return r.host_key
    first = use()
    assert first == 1 and use() == first
    with torch.no_grad():
        next(dynamic.parameters()).add_(1.0)                 # a model that is not retained
    assert use() == first
    with torch.no_grad():
        next(model0.parameters()).add_(1.0)                  # in place under no_grad: the version counter moves
    assert use() == first + 1 and use() == first + 1
    next(model0.parameters()).data.mul_(2.0)                 # behind autograd's back: weights_changed() is the contract
    comp.weights_changed()
    assert use() == first + 2
    comp.after_graph_replay()                                # a replayed training graph moved the values on the device
    assert use() == first + 3
    # detach, change the weights, let a plain call see (and re-pack) them, re-attach: the epoch still moves
    comp.retained = None
    comp.weights_changed()
    comp._retained_weights_key(everything)                   # (whatever another Retained or a plain call looked at in between)
    comp.retained = r
    assert use() == first + 4
    other = comp.retain_objects()
    comp.retained = other
    with torch.no_grad():
        next(model0.parameters()).add_(1.0)
    other.weights_seen(comp._retained_weights_key(other))
    comp.retained = r
    assert use() == first + 5
    assert "weights_seen" in inspect.getsource(ObjectComposer._render)
    # a grid on a retained object must fit the cache's copy of its bits: refused when the call is prepared, by name
    comp.occupancy = comp.occupancy_from_mask({0: torch.ones(1, 65, 64, 64, dtype=torch.bool)})
    with torch.no_grad(), pytest.raises(ValueError, match=r"object 0 is retained.*64\^3"):
        comp._retention_for_call(False, False, None)
    comp.occupancy = comp.occupancy_from_mask({0: torch.ones(1, 64, 64, 64, dtype=torch.bool), K - 1: torch.ones(1, 65, 64, 64, dtype=torch.bool)})
    with torch.no_grad():
        assert comp._retention_for_call(False, False, None) is r          # (64^3 fits; the large grid is on an object that is not retained)
    comp.occupancy = None
    # signatures of recorded frames carry the serial; clearing moves it
    from playableenvironments_amd import environment_model, frame_graph
    assert "retained" in inspect.getsource(frame_graph.FrameGraph._signature)
    assert "retained" in inspect.getsource(environment_model.EnvironmentModel._replay_signature)
    before = r.signature()
    r.clear()
    assert r.signature() != before and r.bytes == 0
    # replicas and copies start without retention
    assert comp._replicate_for_data_parallel().retained is None
    assert copy.deepcopy(comp).retained is None and comp.retained is r
    # a call that the workspace budget splits renders without retention and says so once
    assert "warn_split" in inspect.getsource(ObjectComposer._render)
    with pytest.warns(UserWarning, match="split along the rays"):
        r.warn_split()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r.warn_split()

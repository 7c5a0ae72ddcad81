"""Deferred projection (PR_FLAG_DEFER_PROJECTION), host side: the flag in the header and the binding, the workspace plan, the
composer's switch and the recordings' signatures.  No device work."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from playableenvironments_amd import ObjectComposer, _lib, configs
from tests.test_occupancy_cpu import _host_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_header_and_binding():
    header = open(os.path.join(ROOT, "include", "playrender.h")).read()
    flags = {name: int(value) for name, value in re.findall(r"#define (PR_FLAG_\w+)\s+(\d+)u", header)}
    assert flags["PR_FLAG_DEFER_PROJECTION"] == 2048 == _lib.PR_FLAG_DEFER_PROJECTION
    assert len(set(flags.values())) == len(flags)                          # the next free bit: no flag shares it
    assert all(v & (v - 1) == 0 for v in flags.values())
    assert re.search(r"#define PR_ABI_VERSION 5\b", header)                # existing structs and entry points are unchanged


def _workspace(lib, call, objs):
    size = C.c_size_t()
    assert lib.pr_workspace_size(C.byref(call), objs, C.byref(size)) == 0, lib.pr_last_error()
    return size.value


def _up(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("world,use_fine", [("tennis", False), ("tennis", True), ("minecraft", False), ("reduced", True)])
def test_workspace_grows_by_the_pooled_region_minus_the_narrower_rows(built_library, world, use_fine):
    """With the flag honoured the plan adds 2 K pooled rows of hidden_row_floats(W / 2) floats per ray and sizes the feature arena
    from that row width instead of F; with the flag ignored (sigmoid, training, differentiable, scalar kernel, split precision) the
    size is the unflagged one to the byte."""
    lib = built_library
    cfg = {"tennis": configs.tennis_config, "minecraft": configs.minecraft_config,
           "reduced": lambda: configs.reduced_config(configs.tennis_config())}[world]()
    if use_fine:
        cfg = configs.enable_fine(cfg)
    comp = ObjectComposer(cfg)
    K = comp.object_id_helper.objects_count
    call, objs = _host_call(comp, K, use_fine=use_fine)
    call.flags = _lib.PR_FLAG_GATE_HEAD
    plain = _workspace(lib, call, objs)
    call.flags = _lib.PR_FLAG_GATE_HEAD | _lib.PR_FLAG_DEFER_PROJECTION
    deferred = _workspace(lib, call, objs)
    rays = call.frames * call.rays
    width = objs[0].coarse.layers_width
    F = objs[0].coarse.output_features
    row = _up(width // 2 + 1, 4)
    pooled = _up(4 * 2 * K * rays * row, 256)

    def arena(floats_per_row):
        per_type = []
        for fine in ([False, True] if use_fine else [False]):
            per_type.append(sum(_up(4 * rays * (objs[k].fine if fine else objs[k].coarse).positions * floats_per_row, 256) for k in range(K)))
        return max(per_type)
    assert deferred - plain == pooled + arena(row) - arena(F), (deferred - plain, pooled, arena(row), arena(F))
    for ignored in (_lib.PR_FLAG_SIGMOID_FEATURES, _lib.PR_FLAG_TRAIN_BN, _lib.PR_FLAG_SAVE_FOR_BACKWARD, _lib.PR_FLAG_NAIVE_MLP):
        call.flags = ignored
        without = _workspace(lib, call, objs)
        call.flags = ignored | _lib.PR_FLAG_DEFER_PROJECTION
        assert _workspace(lib, call, objs) == without, ignored
    call.flags = 0
    call.precision = 1                                                     # PR_PRECISION_F16X3: the split kernels write full rows
    without = _workspace(lib, call, objs)
    call.flags = _lib.PR_FLAG_DEFER_PROJECTION
    assert _workspace(lib, call, objs) == without
    call.precision = 0
    call.flags = _lib.PR_FLAG_DEFER_PROJECTION | _lib.PR_FLAG_PERTURB       # perturbed calls are eligible
    assert _workspace(lib, call, objs) - _workspace_without(lib, call, objs) == pooled + arena(row) - arena(F)


def _workspace_without(lib, call, objs):
    flags = call.flags
    call.flags = flags & ~_lib.PR_FLAG_DEFER_PROJECTION
    try:
        return _workspace(lib, call, objs)
    finally:
        call.flags = flags


def test_packed_size_holds_the_projection_matrix(built_library):
    """pr_packed_size accounts for the [W6 | b6] rows (Fpad rows of round_up(W / 2 + 1, 8) floats) in every packing."""
    comp = ObjectComposer(configs.tennis_config())
    s = comp._model_struct(comp.object_models_coarse[2], 32)
    size = C.c_size_t()
    assert built_library.pr_packed_size(C.byref(s), C.byref(size)) == 0
    narrow = comp._model_struct(comp.object_models_coarse[2], 32)
    narrow.output_features = 160                                           # Fpad 192 -> 160: the sizes of head 6 alone change
    small = C.c_size_t()
    assert built_library.pr_packed_size(C.byref(narrow), C.byref(small)) == 0
    w2 = s.layers_width // 2
    w2pad = _up(w2, 32)
    per_block = 32 * (w2pad + 1 + w2pad + _up(w2 + 1, 8))                   # forward fragments, bias, W^T fragments, [W6 | b6] rows
    assert size.value - small.value == 4 * per_block


def test_switch_defaults_on_and_reaches_the_signatures():
    comp = ObjectComposer(configs.tennis_config())
    assert comp.defer_feature_projection is True and comp.gate_feature_head is True
    import inspect
    from playableenvironments_amd import environment_model, frame_graph
    assert "defer_feature_projection" in inspect.getsource(environment_model.EnvironmentModel._replay_signature)
    assert "defer_feature_projection" in inspect.getsource(frame_graph.FrameGraph._signature)
    assert "PR_FLAG_DEFER_PROJECTION" in inspect.getsource(ObjectComposer)


def test_plain_c_client_sees_the_flag(built_library, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    source = tmp_path / "client.c"
    source.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "playrender.h"
int main(void) {
    pr_call_t call;
    memset(&call, 0, sizeof call);
    call.flags = PR_FLAG_GATE_HEAD | PR_FLAG_DEFER_PROJECTION;
    if (pr_abi_version() != PR_ABI_VERSION) return 1;
    printf("flags %u\n", (unsigned)call.flags);
    return 0;
}
""")
    lib_dir = os.path.dirname(_lib.library_path())
    binary = tmp_path / "client"
    build = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(source),
                            "-L", lib_dir, "-lplayrender", f"-Wl,-rpath,{lib_dir}", "-o", str(binary)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "flags 2112" in run.stdout, (run.returncode, run.stdout, run.stderr[-2000:])

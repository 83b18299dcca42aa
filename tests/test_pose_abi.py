"""CPU: the posed-mesh verbs (uh_set_mesh_skin, uh_set_mesh_morph_targets, uh_pose_mesh, uh_get_pose_stats) at the C ABI and in the host
layers - declared and exported, without a group twin, named in the stream-ordering list, refusing a null context without a device, the
stats struct laid out as the header says, the methods present."""
import ctypes as C
import os
import re
import subprocess

import rust_renderer_amd as rr
from rust_renderer_amd.types import PoseStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
VERBS = ("uh_set_mesh_skin", "uh_set_mesh_morph_targets", "uh_pose_mesh", "uh_get_pose_stats")
UH_ERR_INVALID_ARGUMENT = 1


def test_header_declares_and_library_exports_the_verbs():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = rr.load_library()
    for name in VERBS:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name), name
        assert name.replace("uh_", "uh_mgpu_") not in text, "no group twin"
        assert not hasattr(lib, name.replace("uh_", "uh_mgpu_"))


def test_stream_ordering_list_names_the_verbs():
    text = open(HEADER).read()
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    waits = ordering[ordering.index("waits + complete on return"):ordering.index("enqueues like a frame")]
    for name in VERBS:
        assert name in waits, name


def test_null_context_is_refused_without_a_device():
    lib = rr.load_library()
    vp, u32 = C.c_void_p, C.c_uint32
    skin, morph, pose, get = lib.uh_set_mesh_skin, lib.uh_set_mesh_morph_targets, lib.uh_pose_mesh, lib.uh_get_pose_stats
    skin.argtypes, skin.restype = [vp, u32, vp, vp, u32, u32], C.c_int
    morph.argtypes, morph.restype = [vp, u32, vp, vp, u32, u32], C.c_int
    pose.argtypes, pose.restype = [vp, u32, vp, u32, vp, u32], C.c_int
    get.argtypes, get.restype = [vp, C.POINTER(PoseStats)], C.c_int
    joints, floats = (C.c_uint16 * 4)(), (C.c_float * 12)(*([1.0] * 12))
    assert skin(None, 0, joints, floats, 1, 1) == UH_ERR_INVALID_ARGUMENT
    assert skin(None, 0, None, None, 0, 0) == UH_ERR_INVALID_ARGUMENT
    assert morph(None, 0, floats, floats, 1, 1) == UH_ERR_INVALID_ARGUMENT
    assert morph(None, 0, None, None, 0, 0) == UH_ERR_INVALID_ARGUMENT
    assert pose(None, 0, floats, 1, floats, 1) == UH_ERR_INVALID_ARGUMENT
    assert pose(None, 0, None, 0, None, 0) == UH_ERR_INVALID_ARGUMENT
    s = PoseStats()
    assert get(None, C.byref(s)) == UH_ERR_INVALID_ARGUMENT
    assert get(None, None) == UH_ERR_INVALID_ARGUMENT


def test_stats_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in PoseStats._fields_]
    assert fields == ["pose_ms", "poses", "vertices", "joints", "active_targets", "staged_joint_limit", "device_bytes"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu", sizeof(UhPoseStats));\n' +
                   "".join(f'printf(" %zu", offsetof(UhPoseStats, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(PoseStats) == 32
    assert out[1:] == [getattr(PoseStats, f).offset for f in fields]
    assert "UH_LAYOUT_ASSERT(sizeof(UhPoseStats) == 32" in open(HEADER).read()


def test_python_and_cpp_layers_have_the_methods():
    for name in ("set_mesh_skin", "set_mesh_morph_targets", "pose_mesh", "pose_stats"):
        assert callable(getattr(rr.Renderer, name)), name
    assert rr.PoseStats is PoseStats
    host = open(os.path.join(ROOT, "include", "utopian_host.hpp")).read()
    assert "void set_mesh_skin(uint32_t mesh, const uint16_t* joints, const float* weights, uint32_t num_vertices, uint32_t num_joints)" in host
    assert "void set_mesh_morph_targets(uint32_t mesh, const float* position_deltas, const float* normal_deltas, uint32_t num_vertices, uint32_t num_targets)" in host
    assert "void pose_mesh(uint32_t mesh, const float* joint_matrices3x4, uint32_t num_joints, const float* morph_weights = nullptr, uint32_t num_targets = 0)" in host
    assert "UhPoseStats pose_stats()" in host

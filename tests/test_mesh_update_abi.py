"""CPU: uh_update_mesh_vertices / uh_get_mesh_update_stats at the C ABI and in the host layers - exported, named in the stream-ordering
list, refusing a null context without a device, the stats struct laid out as the header says, the methods present."""
import ctypes as C
import os
import re
import subprocess

import rust_renderer_amd as rr
from rust_renderer_amd.types import MeshUpdateStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
VERBS = ("uh_update_mesh_vertices", "uh_get_mesh_update_stats")
UH_ERR_INVALID_ARGUMENT = 1


def test_header_declares_and_library_exports_both_verbs():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = rr.load_library()
    for name in VERBS:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name), name
    assert "uh_mgpu_update_mesh_vertices" not in text  # no group twin, as for the isosurface verbs


def test_header_defines_the_two_places_vertices_may_come_from():
    text = open(HEADER).read()
    assert re.search(r"^#define UH_VERTICES_HOST\s+0\s*$", text, flags=re.M) and re.search(r"^#define UH_VERTICES_DEVICE\s+1\s*$", text, flags=re.M)
    assert (rr.VERTICES_HOST, rr.VERTICES_DEVICE) == (0, 1)


def test_stream_ordering_list_names_both_verbs():
    text = open(HEADER).read()
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    waits = ordering[ordering.index("waits + complete on return"):ordering.index("enqueues like a frame")]
    assert "uh_update_mesh_vertices" in waits and "uh_get_mesh_update_stats" in waits


def test_null_context_is_refused_without_a_device():
    lib = rr.load_library()
    up = lib.uh_update_mesh_vertices
    up.argtypes, up.restype = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int], C.c_int
    vertex = (C.c_uint8 * 80)()
    for where in (0, 1, 2):
        assert up(None, 0, vertex, 1, where) == UH_ERR_INVALID_ARGUMENT
        assert up(None, 0, None, 0, where) == UH_ERR_INVALID_ARGUMENT
    get = lib.uh_get_mesh_update_stats
    get.argtypes, get.restype = [C.c_void_p, C.POINTER(MeshUpdateStats)], C.c_int
    s = MeshUpdateStats()
    assert get(None, C.byref(s)) == UH_ERR_INVALID_ARGUMENT
    assert get(None, None) == UH_ERR_INVALID_ARGUMENT


def test_stats_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in MeshUpdateStats._fields_]
    assert fields == ["gather_ms", "refit_ms", "updates", "triangles", "host_geometry_bytes", "device_bytes"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu", sizeof(UhMeshUpdateStats));\n' +
                   "".join(f'printf(" %zu", offsetof(UhMeshUpdateStats, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(MeshUpdateStats) == 32
    assert out[1:] == [getattr(MeshUpdateStats, f).offset for f in fields]
    assert "UH_LAYOUT_ASSERT(sizeof(UhMeshUpdateStats) == 32" in open(HEADER).read()


def test_python_and_cpp_layers_have_the_methods():
    assert callable(getattr(rr.Renderer, "update_mesh_vertices")) and callable(getattr(rr.Renderer, "mesh_update_stats"))
    assert rr.MeshUpdateStats is MeshUpdateStats
    host = open(os.path.join(ROOT, "include", "utopian_host.hpp")).read()
    assert "void update_mesh_vertices(uint32_t mesh, const UhVertex* vertices, uint32_t num_vertices, int where = UH_VERTICES_HOST)" in host
    assert "UhMeshUpdateStats mesh_update_stats()" in host

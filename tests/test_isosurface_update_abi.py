"""CPU: uh_update_isosurface_mesh / uh_get_isosurface_update_stats at the C ABI and in the Python layer - exported, refusing a null
context without a device, the stats struct laid out as the header says, the methods present."""
import ctypes as C
import os
import re
import subprocess

import rust_renderer_amd as rr
from rust_renderer_amd.types import IsosurfaceUpdateStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
VERBS = ("uh_update_isosurface_mesh", "uh_get_isosurface_update_stats")
UH_ERR_INVALID_ARGUMENT = 1


def test_header_declares_and_library_exports_both_verbs():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = rr.load_library()
    for name in VERBS:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name), name
    assert "uh_mgpu_update_isosurface_mesh" not in text  # no group twin: uh_add_isosurface_mesh has none either


def test_stream_ordering_list_names_the_verb():
    text = open(HEADER).read()
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    assert "uh_update_isosurface_mesh" in ordering and "uh_get_isosurface_update_stats" in ordering


def test_null_context_is_refused_without_a_device():
    lib = rr.load_library()
    up = lib.uh_update_isosurface_mesh
    up.argtypes, up.restype = [C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)], C.c_int
    tris = C.c_uint32(77)
    assert up(None, 0, 0.0, C.byref(tris)) == UH_ERR_INVALID_ARGUMENT
    assert up(None, 0, 0.0, None) == UH_ERR_INVALID_ARGUMENT
    assert tris.value == 77
    get = lib.uh_get_isosurface_update_stats
    get.argtypes, get.restype = [C.c_void_p, C.POINTER(IsosurfaceUpdateStats)], C.c_int
    s = IsosurfaceUpdateStats()
    assert get(None, C.byref(s)) == UH_ERR_INVALID_ARGUMENT
    assert get(None, None) == UH_ERR_INVALID_ARGUMENT


def test_stats_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in IsosurfaceUpdateStats._fields_]
    assert fields == ["extract_ms", "scatter_ms", "updates", "triangles", "host_geometry_bytes", "device_bytes"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu", sizeof(UhIsosurfaceUpdateStats));\n' +
                   "".join(f'printf(" %zu", offsetof(UhIsosurfaceUpdateStats, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(IsosurfaceUpdateStats) == 32
    assert out[1:] == [getattr(IsosurfaceUpdateStats, f).offset for f in fields]
    assert "UH_LAYOUT_ASSERT(sizeof(UhIsosurfaceUpdateStats) == 32" in open(HEADER).read()


def test_python_and_cpp_layers_have_the_methods():
    assert callable(getattr(rr.Renderer, "update_isosurface_mesh")) and callable(getattr(rr.Renderer, "isosurface_update_stats"))
    assert rr.IsosurfaceUpdateStats is IsosurfaceUpdateStats
    host = open(os.path.join(ROOT, "include", "utopian_host.hpp")).read()
    assert "uint32_t update_isosurface_mesh(uint32_t mesh, float time)" in host and "UhIsosurfaceUpdateStats isosurface_update_stats()" in host

"""CPU: the reservoir lights of the hybrid frame (UH_HYBRID_RESTIR_LIGHTS, UH_HYBRID_LIGHT_VISIBILITY, UhHybridRestirStats,
uh_get_hybrid_restir_stats) at the C ABI, in the C++ host header and in the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")


def test_header_declares_the_bit_the_image_and_the_verb():
    text = open(HEADER).read()
    for s in ("UH_HYBRID_RESTIR_LIGHTS = 1u << 12", "UH_HYBRID_LIGHT_VISIBILITY = 13",
              "int uh_get_hybrid_restir_stats(uh_ctx* ctx, UhHybridRestirStats* out);"):
        assert s in text, s
    assert text.index("uh_mgpu_set_option(") < text.index("uh_get_hybrid_restir_stats("), "a per-context verb: after the group section"
    assert "uh_mgpu_get_hybrid_restir_stats" not in text
    assert "1u << 9" not in text, "bit 9 stays unused"
    assert "SAME CAMERA" in text, "the header says whose job the reservoirs' camera is"


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_stats_layout_guard_compiles_as_c_and_matches_ctypes(tmp_path, std):
    src = tmp_path / "r.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(UhHybridRestirStats), offsetof(UhHybridRestirStats, rays), '
                   'offsetof(UhHybridRestirStats, occluded), offsetof(UhHybridRestirStats, pass_ms), offsetof(UhHybridRestirStats, reserved), '
                   'UH_HYBRID_RESTIR_LIGHTS, UH_HYBRID_LIGHT_VISIBILITY); return 0; }\n')
    exe = tmp_path / "r"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = rr.HybridRestirStats
    assert out == [C.sizeof(S), S.rays.offset, S.occluded.offset, S.pass_ms.offset, S.reserved.offset, rr.HYBRID_RESTIR_LIGHTS,
                   rr.HYBRID_LIGHT_VISIBILITY] == [32, 0, 8, 16, 20, 4096, 13]
    # the guard fires on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Duint64_t=uint32_t", "-include", "stdint.h", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")],
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "UhHybridRestirStats" in bad.stderr


def test_host_header_reads_the_image_as_bytes_and_has_the_stats(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() { UhHybridRestirStats (utopian::Renderer::*f)() = &utopian::Renderer::hybrid_restir_stats; return f ? 0 : 1; }\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "which == UH_HYBRID_SHADOWS || which == UH_HYBRID_LIGHT_VISIBILITY) ? 1" in open(os.path.join(INCLUDE, "utopian_host.hpp")).read()


def test_library_exports_the_verb_and_rejects_null():
    lib = rr.load_library()
    assert hasattr(lib, "uh_get_hybrid_restir_stats")
    lib.uh_get_hybrid_restir_stats.argtypes, lib.uh_get_hybrid_restir_stats.restype = [C.c_void_p, C.c_void_p], C.c_int
    s = rr.HybridRestirStats()
    assert lib.uh_get_hybrid_restir_stats(None, C.byref(s)) == 1
    assert not hasattr(lib, "uh_mgpu_get_hybrid_restir_stats")


def test_python_layer_and_the_oracle_renderer():
    assert rr.HYBRID_RESTIR_LIGHTS == 1 << 12 and rr.HYBRID_LIGHT_VISIBILITY == 13
    assert rr.HYBRID_RESTIR_LIGHTS & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER | 1 << 9) == 0
    assert rr.Renderer._HYBRID_IMAGES[rr.HYBRID_LIGHT_VISIBILITY] == (np.uint8, 1)
    assert [f[0] for f in rr.HybridRestirStats._fields_] == ["rays", "occluded", "pass_ms", "reserved"]
    o = oa.OracleRenderer(8, 8)
    with pytest.raises(NotImplementedError):
        o.hybrid_restir_stats()
    with pytest.raises(NotImplementedError):
        o.read_hybrid(rr.HYBRID_LIGHT_VISIBILITY)

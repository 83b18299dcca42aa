"""CPU: motion vectors (UH_HYBRID_MOTION, UH_HYBRID_MOTION_IMAGE, UH_DENOISE_MOTION, UhMotionStats, uh_get_motion_stats) at the C ABI, in
the C++ host header and in the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
STATS = ("pixels_with", "pixels_without", "meshes_static", "meshes_rigid", "meshes_deformed", "meshes_none", "motion_ms", "snapshot_ms")


def test_header_declares_the_bits_the_image_the_verb_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_MOTION = 1u << 14 };", "enum { UH_HYBRID_MOTION_IMAGE = 15", "enum { UH_DENOISE_MOTION = 1u << 3",
              "int uh_get_motion_stats(uh_ctx* ctx, UhMotionStats* out);"):
        assert s in text, s
    assert "1u << 9" not in text, "bit 9 stays unused"
    assert "uh_mgpu_get_motion_stats" not in text
    section = text[text.index("---- motion vectors"):]
    for s in ("static", "rigid", "deformed", "none", "prev_o2w", "b0 = 1 - u - v", "RESOURCES", "STREAM ORDER", "ISOLATION", "UH_DENOISE_MOTION",
              "rebuild_tlas = 1"):
        assert s in section, s
    denoiser = text[text.index("---- the denoiser"):text.index("---- ray-traced ambient occlusion")]
    for s in ("UH_DENOISE_MOTION", "UH_HYBRID_MOTION", "acos(reproject_normal_cos)", "w == 0", "the history follows the moved mesh"):
        assert s in denoiser, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    assert "uh_get_motion_stats" in ordering


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu ", sizeof(UhMotionStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhMotionStats, {f}));\n' for f in STATS) +
                   'printf("%u %d %u\\n", (unsigned)UH_HYBRID_MOTION, UH_HYBRID_MOTION_IMAGE, (unsigned)UH_DENOISE_MOTION); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = rr.MotionStats
    assert out == [C.sizeof(S)] + [getattr(S, f).offset for f in STATS] + [rr.HYBRID_MOTION, rr.HYBRID_MOTION_IMAGE, rr.DENOISE_MOTION]
    assert out == [32, 0, 4, 8, 12, 16, 20, 24, 28, 1 << 14, 15, 8]
    # the guard fires on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhMotionStats" in bad.stderr


def test_host_header_has_the_member_and_sizes_image_15(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhMotionStats (utopian::Renderer::*a)() = &utopian::Renderer::motion_stats;\n"
                   "   return a ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    host = open(os.path.join(INCLUDE, "utopian_host.hpp")).read()
    assert 'static_assert(UH_HYBRID_MOTION_IMAGE == 15, "read_hybrid sizes image 15 as 16-byte texels");' in host
    read = host[host.index("std::vector<uint8_t> read_hybrid(int which)"):host.index("UhHybridStats hybrid_stats()")]
    for narrower in ("UH_HYBRID_AO_COUNTS", "UH_HYBRID_SSAO_IMAGE", "UH_HYBRID_ALBEDO"):
        assert narrower in read
    assert "UH_HYBRID_MOTION_IMAGE) ?" not in read and ": 16;" in read, "image 15 falls to the 16-byte texels"


def test_library_exports_the_verb_and_no_group_twin():
    lib = rr.load_library()
    assert hasattr(lib, "uh_get_motion_stats") and not hasattr(lib, "uh_mgpu_get_motion_stats")


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    lib.uh_get_motion_stats.argtypes, lib.uh_get_motion_stats.restype = [C.c_void_p, C.c_void_p], C.c_int
    s = rr.MotionStats()
    assert lib.uh_get_motion_stats(None, C.byref(s)) == 1 and lib.uh_get_motion_stats(None, None) == 1


def test_python_layer():
    assert rr.HYBRID_MOTION == 1 << 14 and rr.HYBRID_MOTION_IMAGE == 15 and rr.DENOISE_MOTION == 8
    assert rr.HYBRID_MOTION & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                               rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | 1 << 9) == 0
    assert rr.DENOISE_MOTION & (rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE | 4) == 0
    assert rr.Renderer._HYBRID_IMAGES[rr.HYBRID_MOTION_IMAGE] == (np.float32, 4)
    assert sorted(rr.Renderer._HYBRID_IMAGES) == list(range(16))
    assert [f[0] for f in rr.MotionStats._fields_] == list(STATS)
    assert callable(rr.Renderer.motion_stats)
    # the denoiser's own refusal is unchanged: bit 2 alone is not a flag of the Python layer either
    assert all(getattr(rr, n) != 4 for n in dir(rr) if n.startswith("DENOISE_") and n in ("DENOISE_TEMPORAL", "DENOISE_DEMODULATE", "DENOISE_MOTION"))

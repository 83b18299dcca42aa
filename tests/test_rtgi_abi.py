"""CPU: one-bounce ray-traced diffuse GI (UH_HYBRID_RTGI, UH_HYBRID_GI_RADIANCE, UH_HYBRID_GI_COUNTS, UhRtgiParams, UhRtgiStats,
uh_rtgi_default_params, uh_set_rtgi_params, uh_get_rtgi_stats) at the C ABI, in the C++ host header and in the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtgi_reference as gi
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
VERBS = ("uh_rtgi_default_params", "uh_set_rtgi_params", "uh_get_rtgi_stats")
FIELDS = ("samples", "blur_radius", "max_radiance", "intensity", "blur_normal_cos", "blur_plane")
STATS = ("pixels", "rays", "shadow_rays", "misses", "trace_ms", "shadow_ms", "filter_ms", "composite_ms")


def test_header_declares_the_bit_the_images_the_verbs_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_RTGI = 1u << 17 };", "UH_HYBRID_GI_RADIANCE = 18", "UH_HYBRID_GI_COUNTS = 19", "int uh_rtgi_default_params(UhRtgiParams* out);",
              "int uh_set_rtgi_params(uh_ctx* ctx, const UhRtgiParams* params);", "int uh_get_rtgi_stats(uh_ctx* ctx, UhRtgiStats* out);"):
        assert s in text, s
    assert "1u << 9" not in text, "bit 9 stays unused"
    assert "uh_mgpu_set_rtgi_params" not in text
    section = text[text.index("---- one-bounce ray-traced diffuse GI"):]
    for s in ("EXTENSION", "0x52544749", "0.03 ambient STAYS", "G-buffer orientation", "STREAM ORDER", "ISOLATION", "OUT OF SCOPE", "ibl_enabled == 1",
              "UH_HYBRID_DEFERRED", "No uh_mgpu_ twin"):
        assert s in section, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in ("uh_set_rtgi_params", "uh_get_rtgi_stats", "uh_rtgi_default_params"):
        assert verb in ordering, verb


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhRtgiParams), sizeof(UhRtgiStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhRtgiParams, {f}));\n' for f in FIELDS) +
                   "".join(f'printf("%zu ", offsetof(UhRtgiStats, {f}));\n' for f in STATS) +
                   'printf("%u %d %d\\n", (unsigned)UH_HYBRID_RTGI, UH_HYBRID_GI_RADIANCE, UH_HYBRID_GI_COUNTS); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.RtgiParams, rr.RtgiStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATS] + \
        [rr.HYBRID_RTGI, rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS]
    assert out == [24, 48, 0, 4, 8, 12, 16, 20, 0, 8, 16, 24, 32, 36, 40, 44, 1 << 17, 18, 19]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhRtgiParams" in bad.stderr and "UhRtgiStats" in bad.stderr


def test_host_header_has_the_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhRtgiParams (*a)() = &utopian::Renderer::default_rtgi_params;\n"
                   "   void (utopian::Renderer::*b)(const UhRtgiParams&) = &utopian::Renderer::set_rtgi_params;\n"
                   "   UhRtgiStats (utopian::Renderer::*c)() = &utopian::Renderer::rtgi_stats;\n"
                   "   return a && b && c ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "which == UH_HYBRID_GI_COUNTS" in open(os.path.join(INCLUDE, "utopian_host.hpp")).read(), "read_hybrid sizes image 19 as four bytes"


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_match_the_restatement():
    p = rr.rtgi_default_params()
    assert (p.samples, p.blur_radius, p.max_radiance, p.intensity) == (2, 3, 16.0, 1.0)
    assert p.blur_normal_cos == np.float32(0.9) and p.blur_plane == np.float32(0.05)
    assert {f: np.float32(getattr(p, f)) for f in FIELDS} == {k: np.float32(v) for k, v in gi.default_params().items()}


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    lib.uh_rtgi_default_params.argtypes, lib.uh_rtgi_default_params.restype = [vp], C.c_int
    assert lib.uh_rtgi_default_params(None) == 1
    lib.uh_set_rtgi_params.argtypes, lib.uh_set_rtgi_params.restype = [vp, vp], C.c_int
    p = rr.rtgi_default_params()
    assert lib.uh_set_rtgi_params(None, C.byref(p)) == 1 and lib.uh_set_rtgi_params(None, None) == 1
    lib.uh_get_rtgi_stats.argtypes, lib.uh_get_rtgi_stats.restype = [vp, vp], C.c_int
    s = rr.RtgiStats()
    assert lib.uh_get_rtgi_stats(None, C.byref(s)) == 1 and lib.uh_get_rtgi_stats(None, None) == 1


def test_python_layer():
    assert rr.HYBRID_RTGI == 1 << 17 and (rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS) == (18, 19)
    assert rr.HYBRID_RTGI & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                             rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | rr.HYBRID_MOTION | rr.HYBRID_TAA | rr.HYBRID_POST | 1 << 9) == 0
    assert rr.Renderer._GI_IMAGES == {rr.HYBRID_GI_RADIANCE: (np.float32, 4), rr.HYBRID_GI_COUNTS: (np.uint8, 4)}
    assert [f[0] for f in rr.RtgiParams._fields_] == list(FIELDS) and [f[0] for f in rr.RtgiStats._fields_] == list(STATS)
    assert callable(rr.Renderer.set_rtgi_params) and callable(rr.Renderer.rtgi_stats)

"""CPU: emissive meshes as area lights (UH_HYBRID_AREA_LIGHTS, UH_HYBRID_AREA_DIFFUSE / SPECULAR / COUNTS, UhAreaLightParams,
UhAreaLightStats, uh_area_light_default_params, uh_set_area_light_params, uh_get_area_light_stats, uh_read_area_emitters) at the C ABI and
in the Python layer: layouts through the C compiler and ctypes, the defaults, every parameter rule's text and order, the null arguments,
and the header section's paragraphs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import area_light_reference as al
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
CSRC = os.path.join(ROOT, "rust-renderer_amd", "csrc")
VERBS = ("uh_area_light_default_params", "uh_set_area_light_params", "uh_get_area_light_stats", "uh_read_area_emitters")
FIELDS = ("samples", "blur_radius", "show_emitters", "max_weight", "max_radiance", "intensity", "blur_normal_cos", "blur_plane")
STATS = ("pixels", "samples", "shadow_rays", "occluded", "emitter_pixels", "emitters", "total_weight", "table_builds", "table_ms", "sample_ms", "shadow_ms",
         "filter_ms", "composite_ms", "reserved")


def test_header_declares_the_bit_the_images_the_verbs_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_AREA_LIGHTS = 1u << 21 };", "UH_HYBRID_AREA_DIFFUSE = 28", "UH_HYBRID_AREA_SPECULAR = 29", "UH_HYBRID_AREA_COUNTS = 30",
              "int uh_area_light_default_params(UhAreaLightParams* out);", "int uh_set_area_light_params(uh_ctx* ctx, const UhAreaLightParams* params);",
              "int uh_get_area_light_stats(uh_ctx* ctx, UhAreaLightStats* out);",
              "int uh_read_area_emitters(uh_ctx* ctx, uint32_t capacity, uint32_t* keys, float* areas, uint32_t* weights, uint32_t* count);"):
        assert s in text, s
    assert "uh_mgpu_set_area_light_params" not in text
    section = text[text.index("---- emissive meshes as area lights"):]
    for s in ("EXTENSION", "0x41524541", "directly AFTER the deferred pass and BEFORE the rtgi pass", "G-buffer orientation", "PARAMS", "READ-BACK", "RESOURCES",
              "STREAM ORDER", "ISOLATION", "OUT OF SCOPE", "UH_HYBRID_DEFERRED", "UH_ERR_CAPACITY", "UH_ERR_NOT_BUILT", "no ibl_enabled rule", "No uh_mgpu_ twin",
              "allocates nothing", "emissiveFactor", "2^20 emitter triangles"):
        assert s in section, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in VERBS:
        assert verb in ordering, verb


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhAreaLightParams), sizeof(UhAreaLightStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhAreaLightParams, {f}));\n' for f in FIELDS) +
                   "".join(f'printf("%zu ", offsetof(UhAreaLightStats, {f}));\n' for f in STATS) +
                   'printf("%u %d %d %d\\n", (unsigned)UH_HYBRID_AREA_LIGHTS, UH_HYBRID_AREA_DIFFUSE, UH_HYBRID_AREA_SPECULAR, UH_HYBRID_AREA_COUNTS); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.AreaLightParams, rr.AreaLightStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATS] + \
        [rr.HYBRID_AREA_LIGHTS, rr.HYBRID_AREA_DIFFUSE, rr.HYBRID_AREA_SPECULAR, rr.HYBRID_AREA_COUNTS]
    assert out == [32, 88] + list(range(0, 32, 4)) + list(range(0, 64, 8)) + [64, 68, 72, 76, 80, 84] + [1 << 21, 28, 29, 30]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhAreaLightParams" in bad.stderr and "UhAreaLightStats" in bad.stderr


def test_host_header_has_the_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhAreaLightParams (*a)() = &utopian::Renderer::default_area_light_params;\n"
                   "   void (utopian::Renderer::*b)(const UhAreaLightParams&) = &utopian::Renderer::set_area_light_params;\n"
                   "   UhAreaLightStats (utopian::Renderer::*c)() = &utopian::Renderer::area_light_stats;\n"
                   "   utopian::Renderer::AreaEmitters (utopian::Renderer::*d)() = &utopian::Renderer::read_area_emitters;\n"
                   "   return a && b && c && d ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "which == UH_HYBRID_AREA_COUNTS" in open(os.path.join(INCLUDE, "utopian_host.hpp")).read(), "read_hybrid sizes image 30 as four bytes"


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_match_the_restatement():
    p = rr.area_light_default_params()
    assert (p.samples, p.blur_radius, p.show_emitters, p.max_weight, p.max_radiance, p.intensity) == (2, 3, 1, 64.0, 16.0, 1.0)
    assert p.blur_normal_cos == np.float32(0.9) and p.blur_plane == np.float32(0.05)
    assert {f: np.float32(getattr(p, f)) for f in FIELDS} == {k: np.float32(v) for k, v in al.default_params().items()}


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    lib.uh_area_light_default_params.argtypes, lib.uh_area_light_default_params.restype = [vp], C.c_int
    assert lib.uh_area_light_default_params(None) == 1
    lib.uh_set_area_light_params.argtypes, lib.uh_set_area_light_params.restype = [vp, vp], C.c_int
    p = rr.area_light_default_params()
    assert lib.uh_set_area_light_params(None, C.byref(p)) == 1 and lib.uh_set_area_light_params(None, None) == 1
    lib.uh_get_area_light_stats.argtypes, lib.uh_get_area_light_stats.restype = [vp, vp], C.c_int
    s = rr.AreaLightStats()
    assert lib.uh_get_area_light_stats(None, C.byref(s)) == 1 and lib.uh_get_area_light_stats(None, None) == 1
    lib.uh_read_area_emitters.argtypes, lib.uh_read_area_emitters.restype = [vp, C.c_uint32, vp, vp, vp, vp], C.c_int
    n = C.c_uint32()
    assert lib.uh_read_area_emitters(None, 0, None, None, None, C.byref(n)) == 1


def test_the_refusals_carry_these_texts():
    """the message texts of uh_set_area_light_params' rules and of uh_read_hybrid's refusal of images 28..30, as the library's sources state
    them. Their order by behaviour is tests/cpp/area_light_plan_check.cpp's (the plan rules) and, on a context, tests/test_gpu_area_lights.py's
    (every parameter refusal, with the old params kept: set_params needs a context, which needs a device)"""
    passes = open(os.path.join(CSRC, "hybrid_ray_passes.hip")).read()
    for s in ("samples must be 1..16", "blur_radius must be 0..6", "show_emitters must be 0 or 1", "max_weight must be finite and > 0",
              "max_radiance must be finite and > 0", "intensity must be finite and >= 0", "blur_normal_cos and blur_plane must not be NaN"):
        assert s in passes, s
    verbs = open(os.path.join(CSRC, "hybrid_verbs.hip")).read()
    assert "images 28..30 before the first area-light pass (UH_HYBRID_AREA_LIGHTS); until then the image index must be 0..27" in verbs
    assert "image index must be 0..30" in verbs


def test_python_layer():
    assert rr.HYBRID_AREA_LIGHTS == 1 << 21 and (rr.HYBRID_AREA_DIFFUSE, rr.HYBRID_AREA_SPECULAR, rr.HYBRID_AREA_COUNTS) == (28, 29, 30)
    assert rr.HYBRID_AREA_LIGHTS & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                                    rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | rr.HYBRID_MOTION | rr.HYBRID_TAA | rr.HYBRID_POST | rr.HYBRID_RTGI |
                                    rr.HYBRID_GLOSSY | rr.HYBRID_FOG | rr.HYBRID_GLASS | 1 << 9) == 0
    assert rr.Renderer._AREA_IMAGES == {rr.HYBRID_AREA_DIFFUSE: (np.float32, 4), rr.HYBRID_AREA_SPECULAR: (np.float32, 4), rr.HYBRID_AREA_COUNTS: (np.uint8, 4)}
    assert [f[0] for f in rr.AreaLightParams._fields_] == list(FIELDS) and [f[0] for f in rr.AreaLightStats._fields_] == list(STATS)
    assert callable(rr.Renderer.set_area_light_params) and callable(rr.Renderer.area_light_stats) and callable(rr.Renderer.read_area_emitters)
    from rust_renderer_amd import api

    for verb in VERBS:
        assert verb[3:] in api._SIGNATURES, verb

"""Ray-traced glass (UH_HYBRID_GLASS, UH_HYBRID_GLASS_RADIANCE / _COUNTS / _EVENTS, UhGlassParams, UhGlassStats, uh_glass_default_params,
uh_set_glass_params, uh_get_glass_stats) at the C ABI, in the C++ host header and in the Python layer, and the refusal strings in the
sources. CPU, but for the validation rules of uh_set_glass_params: that verb needs a context, and a context needs a device, so that one
test is marked gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import glass_reference as gs
import rust_renderer_amd as rr
from rust_renderer_amd.api import UtopianError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
CSRC = os.path.join(ROOT, "rust-renderer_amd", "csrc")
VERBS = ("uh_glass_default_params", "uh_set_glass_params", "uh_get_glass_stats")
FIELDS = ("max_events", "max_radiance", "intensity")
STATS = ("pixels", "chains", "segments", "events", "tir", "cut", "shadow_rays", "misses", "trace_ms", "bend_ms", "shadow_ms", "composite_ms")


def test_header_declares_the_bit_the_images_the_verbs_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_GLASS = 1u << 20 };", "UH_HYBRID_GLASS_RADIANCE = 25", "UH_HYBRID_GLASS_COUNTS = 26", "UH_HYBRID_GLASS_EVENTS = 27",
              "int uh_glass_default_params(UhGlassParams* out);", "int uh_set_glass_params(uh_ctx* ctx, const UhGlassParams* params);",
              "int uh_get_glass_stats(uh_ctx* ctx, UhGlassStats* out);"):
        assert s in text, s
    assert "uh_mgpu_set_glass_params" not in text
    section = text[text.index("---- ray-traced glass"):]
    for s in ("REPLACES", "rchit:62-79", "1 / ior on the way OUT", "not textbook Snell", "PARAMS", "READ-BACK", "RESOURCES", "G-buffer orientation", "STREAM ORDER",
              "ISOLATION", "No uh_mgpu_ twin", "bytes per pixel", "bytes per ray", "UH_HYBRID_DEFERRED", "2^27", "no read-back"):
        assert s in section, s
    scope = section[section.index("OUT OF SCOPE"):section.index("Arithmetic:")]
    for s in ("Fresnel split", "absorption or tint", "rough transmission", "point,\n * spot and reservoir lights", "fog inside chains", "marching-cubes mesh",
              "forward graph", "skip glass pixels"):
        assert s in scope, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in VERBS:
        assert verb in ordering, verb
    assert "UH_HYBRID_FOG and UH_HYBRID_GLASS)" in text, "the bit is named among those uh_render_hybrid does not ignore"


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhGlassParams), sizeof(UhGlassStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhGlassParams, {f}));\n' for f in FIELDS) +
                   "".join(f'printf("%zu ", offsetof(UhGlassStats, {f}));\n' for f in STATS) +
                   'printf("%u %d %d %d\\n", (unsigned)UH_HYBRID_GLASS, UH_HYBRID_GLASS_RADIANCE, UH_HYBRID_GLASS_COUNTS, UH_HYBRID_GLASS_EVENTS); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.GlassParams, rr.GlassStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATS] + \
        [rr.HYBRID_GLASS, rr.HYBRID_GLASS_RADIANCE, rr.HYBRID_GLASS_COUNTS, rr.HYBRID_GLASS_EVENTS]
    assert out == [12, 80, 0, 4, 8, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 1 << 20, 25, 26, 27]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhGlassParams" in bad.stderr and "UhGlassStats" in bad.stderr


def test_host_header_has_the_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhGlassParams (*a)() = &utopian::Renderer::default_glass_params;\n"
                   "   void (utopian::Renderer::*b)(const UhGlassParams&) = &utopian::Renderer::set_glass_params;\n"
                   "   UhGlassStats (utopian::Renderer::*c)() = &utopian::Renderer::glass_stats;\n"
                   "   return a && b && c ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    host = open(os.path.join(INCLUDE, "utopian_host.hpp")).read()
    assert "which == UH_HYBRID_GLASS_COUNTS" in host and "which == UH_HYBRID_GLASS_EVENTS" in host, "read_hybrid sizes images 26 and 27 as four bytes"


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_are_the_stated_values():
    p = rr.glass_default_params()
    assert (p.max_events, p.max_radiance, p.intensity) == (8, 16.0, 1.0)
    d = gs.default_params()
    assert all(np.float32(getattr(p, f)) == np.float32(d[f]) for f in FIELDS)


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    lib.uh_glass_default_params.argtypes, lib.uh_glass_default_params.restype = [vp], C.c_int
    assert lib.uh_glass_default_params(None) == 1
    lib.uh_set_glass_params.argtypes, lib.uh_set_glass_params.restype = [vp, vp], C.c_int
    p = rr.glass_default_params()
    assert lib.uh_set_glass_params(None, C.byref(p)) == 1 and lib.uh_set_glass_params(None, None) == 1
    lib.uh_get_glass_stats.argtypes, lib.uh_get_glass_stats.restype = [vp, vp], C.c_int
    s = rr.GlassStats()
    assert lib.uh_get_glass_stats(None, C.byref(s)) == 1 and lib.uh_get_glass_stats(None, None) == 1


def test_python_layer():
    assert rr.HYBRID_GLASS == 1 << 20 and (rr.HYBRID_GLASS_RADIANCE, rr.HYBRID_GLASS_COUNTS, rr.HYBRID_GLASS_EVENTS) == (25, 26, 27)
    assert rr.HYBRID_GLASS & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                              rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | rr.HYBRID_MOTION | rr.HYBRID_TAA | rr.HYBRID_POST | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY |
                              rr.HYBRID_FOG | 1 << 9) == 0
    assert rr.Renderer._GLASS_IMAGES == {rr.HYBRID_GLASS_RADIANCE: (np.float32, 4), rr.HYBRID_GLASS_COUNTS: (np.uint8, 4), rr.HYBRID_GLASS_EVENTS: (np.uint8, 4)}
    assert rr.Renderer._glass_rendered is False, "the three images exist only once a call with the bit has succeeded on that renderer"
    assert [f[0] for f in rr.GlassParams._fields_] == list(FIELDS) and [f[0] for f in rr.GlassStats._fields_] == list(STATS)
    assert callable(rr.Renderer.set_glass_params) and callable(rr.Renderer.glass_stats) and callable(rr.glass_default_params)


def test_the_refusal_strings():
    """what uh_render_hybrid and uh_read_hybrid answer, in the order the header states, behind every older rule; and the older strings stay.
    The plan's rules are text in csrc/hybrid_plan.h (tests/cpp/hybrid_plan_check.cpp asserts their order by behaviour, all 39 of them);
    "uh_render_hybrid before uh_build_acceleration" is no plan rule and is not searched for here: its place behind every plan rule is
    test_gpu_hybrid_refusal_order.py::test_every_refusal_comes_before_not_built's, on the GPU. The params strings stand with the glass
    pass's verbs in csrc/hybrid_ray_passes.hip."""
    plan = open(os.path.join(CSRC, "hybrid_plan.h")).read()
    order = ["UH_HYBRID_FOG: a frame of 2^26 pixels or more",
             "UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1",
             "UH_HYBRID_GLASS casts its rays from the G-buffer, and no G-buffer has been rendered",
             "UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call",
             "UH_HYBRID_GLASS: a frame of 2^27 pixels or more"]
    at = [plan.index(s) for s in order]
    assert at == sorted(at), "the refusals stand in this order in the plan"
    verbs = open(os.path.join(CSRC, "hybrid_verbs.hip")).read()
    assert ('"uh_read_hybrid: images 25..27 before the first glass pass (UH_HYBRID_GLASS); until then the image index must be 0..24"') in verbs
    for s in ("must be 0..17", "images 20..22 before the first glossy pass", "images 23..24 before the first fog pass", "image index must be 0..27"):
        assert s in verbs, s
    passes = open(os.path.join(CSRC, "hybrid_ray_passes.hip")).read()
    for s in ("max_events must be 1..16", "max_radiance must be finite and > 0", "intensity must be finite and >= 0"):
        assert s in passes, s


@pytest.mark.gpu
def test_every_validation_rule_one_field_at_a_time():
    """each rule of uh_set_glass_params with one field off and the others at their defaults; a refused call names the field and leaves
    the old params, which the next pass shows"""
    import hybrid_reference as hr

    scene = gs.nested_boxes_scene()
    gpu = rr.Renderer(gs.W, gs.H)
    hr.upload_recorded(scene, gpu, True)
    kept = gpu.set_glass_params(max_events=2, intensity=0.5)
    nan, inf = float("nan"), float("inf")
    bad = [("max_events", 0), ("max_events", 17), ("max_radiance", 0.0), ("max_radiance", -1.0), ("max_radiance", nan), ("max_radiance", inf),
           ("intensity", -0.5), ("intensity", nan), ("intensity", inf)]
    for field, value in bad:
        with pytest.raises(UtopianError, match=f"uh_set_glass_params: {field}") as e:
            gpu.set_glass_params(**{field: value})
        assert "INVALID_ARGUMENT" in str(e.value), (field, value)
    for ok in (dict(max_events=1), dict(max_events=16), dict(intensity=0.0), dict(max_radiance=1e-30)):
        gpu.set_glass_params(**ok)
    gpu.set_glass_params(kept)
    with pytest.raises(UtopianError, match="uh_set_glass_params: max_events"):
        gpu.set_glass_params(max_events=40, intensity=2.0)
    v = gs.scene_view(scene)
    gpu.render_hybrid(v, rr.HYBRID_FRAME | rr.HYBRID_GLASS)
    s = gpu.glass_stats()
    # max_events = 2: chain 1 reaches the emitter with its second event, chain 0 is cut at the outer box; intensity 0.5
    assert s.pixels == gs.W * gs.H and s.chains == 2 * s.pixels and s.events == s.chains and s.cut == s.pixels
    C_ = gpu.read_hybrid(rr.HYBRID_GLASS_RADIANCE)
    out = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    assert np.array_equal(out[..., :3], C_[..., :3] * np.float32(0.5)) and (C_[..., 3] == 1).all()

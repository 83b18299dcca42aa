"""CPU: ray-traced ambient occlusion (UH_HYBRID_RTAO, UH_HYBRID_AO_COUNTS, UhRtaoParams, UhRtaoStats, uh_rtao_default_params,
uh_set_rtao_params, uh_get_rtao_stats) at the C ABI, in the C++ host header and in the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as oa
import rtao_reference as ao
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
VERBS = ("uh_rtao_default_params", "uh_set_rtao_params", "uh_get_rtao_stats", "uh_get_rtao_visits")
FIELDS = ("samples", "radius", "strength", "blur_radius", "blur_normal_cos", "blur_plane")
STATS = ("pixels", "rays", "occluded", "trace_ms", "filter_ms")


def test_header_declares_the_bit_the_image_the_verbs_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_RTAO = 1u << 13 };", "enum { UH_HYBRID_AO_COUNTS = 14", "int uh_rtao_default_params(UhRtaoParams* out);",
              "int uh_set_rtao_params(uh_ctx* ctx, const UhRtaoParams* params);", "int uh_get_rtao_stats(uh_ctx* ctx, UhRtaoStats* out);",
              "int uh_get_rtao_visits(uh_ctx* ctx, uint64_t* nodes, uint64_t* triangles);"):
        assert s in text, s
    assert "1u << 9" not in text, "bit 9 stays unused"
    assert "uh_mgpu_set_rtao_params" not in text
    section = text[text.index("---- ray-traced ambient occlusion"):]
    for s in ("ssao_enabled", "(x, H - 1 - y)", "bytes per pixel", "STREAM ORDER", "ISOLATION", "blur.frag"):
        assert s in section, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in ("uh_set_rtao_params", "uh_get_rtao_stats"):
        assert verb in ordering, verb


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhRtaoParams), sizeof(UhRtaoStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhRtaoParams, {f}));\n' for f in FIELDS) +
                   "".join(f'printf("%zu ", offsetof(UhRtaoStats, {f}));\n' for f in STATS) +
                   'printf("%u %d\\n", (unsigned)UH_HYBRID_RTAO, UH_HYBRID_AO_COUNTS); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.RtaoParams, rr.RtaoStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATS] + [rr.HYBRID_RTAO, rr.HYBRID_AO_COUNTS]
    assert out == [24, 32, 0, 4, 8, 12, 16, 20, 0, 8, 16, 24, 28, 1 << 13, 14]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhRtaoParams" in bad.stderr and "UhRtaoStats" in bad.stderr


def test_host_header_has_the_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhRtaoParams (*a)() = &utopian::Renderer::default_rtao_params;\n"
                   "   void (utopian::Renderer::*b)(const UhRtaoParams&) = &utopian::Renderer::set_rtao_params;\n"
                   "   UhRtaoStats (utopian::Renderer::*c)() = &utopian::Renderer::rtao_stats;\n"
                   "   return a && b && c ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "which == UH_HYBRID_AO_COUNTS" in open(os.path.join(INCLUDE, "utopian_host.hpp")).read(), "read_hybrid sizes image 14 as bytes"


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_match_the_restatement():
    p = rr.rtao_default_params()
    assert (p.samples, p.radius, p.strength, p.blur_radius) == (4, 1.0, 1.0, 2)
    assert p.blur_normal_cos == np.float32(0.9) and p.blur_plane == np.float32(0.05)
    assert {f: np.float32(getattr(p, f)) for f in FIELDS} == {k: np.float32(v) for k, v in ao.default_params().items()}


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    lib.uh_rtao_default_params.argtypes, lib.uh_rtao_default_params.restype = [vp], C.c_int
    assert lib.uh_rtao_default_params(None) == 1
    lib.uh_set_rtao_params.argtypes, lib.uh_set_rtao_params.restype = [vp, vp], C.c_int
    p = rr.rtao_default_params()
    assert lib.uh_set_rtao_params(None, C.byref(p)) == 1 and lib.uh_set_rtao_params(None, None) == 1
    lib.uh_get_rtao_stats.argtypes, lib.uh_get_rtao_stats.restype = [vp, vp], C.c_int
    s = rr.RtaoStats()
    assert lib.uh_get_rtao_stats(None, C.byref(s)) == 1 and lib.uh_get_rtao_stats(None, None) == 1
    lib.uh_get_rtao_visits.argtypes, lib.uh_get_rtao_visits.restype = [vp, vp, vp], C.c_int
    n = C.c_uint64()
    assert lib.uh_get_rtao_visits(None, C.byref(n), C.byref(n)) == 1


def test_python_layer_and_the_oracle_renderer():
    assert rr.HYBRID_RTAO == 1 << 13 and rr.HYBRID_AO_COUNTS == 14
    assert rr.HYBRID_RTAO & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                             rr.HYBRID_RESTIR_LIGHTS | 1 << 9) == 0
    assert rr.Renderer._HYBRID_IMAGES[rr.HYBRID_AO_COUNTS] == (np.uint8, 1)
    assert [f[0] for f in rr.RtaoParams._fields_] == list(FIELDS) and [f[0] for f in rr.RtaoStats._fields_] == list(STATS)
    o = oa.OracleRenderer(8, 8)
    for call in (o.set_rtao_params, o.rtao_stats, o.rtao_visits):
        with pytest.raises(NotImplementedError):
            call()

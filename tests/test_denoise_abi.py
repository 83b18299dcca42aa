"""CPU: the denoiser (uh_denoise, uh_denoise_default_params, uh_reset_denoise_history, uh_read_denoised, uh_get_denoise_stats,
UhDenoiseParams, UhDenoiseStats) at the C ABI, in the C++ host header and in the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as dr
import oracle_api as oa
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
VERBS = ("uh_denoise_default_params", "uh_denoise", "uh_reset_denoise_history", "uh_read_denoised", "uh_get_denoise_stats")


def test_header_declares_the_verbs_the_images_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_DENOISE_TEMPORAL = 1u << 0, UH_DENOISE_DEMODULATE = 1u << 1 };",
              "int uh_denoise_default_params(UhDenoiseParams* out);",
              "int uh_denoise(uh_ctx* ctx, const UhViewUniformData* view, const UhDenoiseParams* params);",
              "int uh_reset_denoise_history(uh_ctx* ctx);", "int uh_read_denoised(uh_ctx* ctx, int which, void* out);",
              "int uh_get_denoise_stats(uh_ctx* ctx, UhDenoiseStats* out);", "UH_DENOISE_COLOR = 0", "UH_DENOISE_OUTPUT = 1", "UH_DENOISE_INPUT = 2",
              "UH_DENOISE_TEMPORAL_COLOR = 3", "UH_DENOISE_HISTORY = 4", "UH_DENOISE_VARIANCE = 5"):
        assert s in text, s
    assert text.index("uh_get_hybrid_restir_stats(uh_ctx* ctx") < text.index("int uh_denoise("), 'a new section after "Reservoir lights"'
    assert "uh_mgpu_denoise" not in text
    section = text[text.index("---- the denoiser"):]
    for s in ("SAME CAMERA", "bytes per pixel", "uh_reset_denoise_history, or accept", "STREAM ORDER", "ISOLATION"):
        assert s in section, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in ("uh_denoise", "uh_read_denoised", "uh_get_denoise_stats", "uh_reset_denoise_history"):
        assert verb in ordering, verb


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "d.c"
    fields = ("flags", "iterations", "max_history", "alpha_min", "sigma_luminance", "sigma_plane", "reproject_normal_cos", "reproject_plane", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhDenoiseParams), sizeof(UhDenoiseStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhDenoiseParams, {f}));\n' for f in fields) +
                   'printf("%zu %zu %zu %zu ", offsetof(UhDenoiseStats, pass_ms), offsetof(UhDenoiseStats, geometry_pixels), '
                   'offsetof(UhDenoiseStats, history_pixels), offsetof(UhDenoiseStats, reserved));\n'
                   'printf("%d %d %d %d %d %d %d %d\\n", UH_DENOISE_TEMPORAL, UH_DENOISE_DEMODULATE, UH_DENOISE_COLOR, UH_DENOISE_OUTPUT, UH_DENOISE_INPUT, '
                   'UH_DENOISE_TEMPORAL_COLOR, UH_DENOISE_HISTORY, UH_DENOISE_VARIANCE); return 0; }\n')
    exe = tmp_path / "d"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.DenoiseParams, rr.DenoiseStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in fields] + \
        [S.pass_ms.offset, S.geometry_pixels.offset, S.history_pixels.offset, S.reserved.offset] + \
        [rr.DENOISE_TEMPORAL, rr.DENOISE_DEMODULATE, rr.DENOISE_COLOR, rr.DENOISE_OUTPUT, rr.DENOISE_INPUT, rr.DENOISE_TEMPORAL_COLOR,
         rr.DENOISE_HISTORY, rr.DENOISE_VARIANCE]
    assert out == [48, 32, 0, 4, 8, 12, 16, 20, 24, 28, 32, 0, 16, 20, 24, 1, 2, 0, 1, 2, 3, 4, 5]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhDenoiseParams" in bad.stderr and "UhDenoiseStats" in bad.stderr


def test_host_header_has_the_four_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   void (utopian::Renderer::*a)(const UhViewUniformData&, const UhDenoiseParams&) = &utopian::Renderer::denoise;\n"
                   "   void (utopian::Renderer::*a2)(const UhViewUniformData&) = &utopian::Renderer::denoise;\n"
                   "   std::vector<uint8_t> (utopian::Renderer::*b)(int) = &utopian::Renderer::read_denoised;\n"
                   "   void (utopian::Renderer::*c)() = &utopian::Renderer::reset_denoise_history;\n"
                   "   UhDenoiseStats (utopian::Renderer::*d)() = &utopian::Renderer::denoise_stats;\n"
                   "   UhDenoiseParams (*e)() = &utopian::Renderer::default_denoise_params;\n"
                   "   return a && a2 && b && c && d && e ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_match_the_restatement():
    p = rr.default_denoise_params()
    assert p.flags == rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE and p.iterations == 5 and p.max_history == 32
    assert p.alpha_min == np.float32(0.2) and p.sigma_luminance == 4.0 and p.reproject_normal_cos == np.float32(0.9)
    assert p.sigma_plane > 0 and p.reproject_plane > 0 and not any(p.reserved)
    want = dr.default_params()
    assert {k: np.float32(v) for k, v in dr.params_of(p).items()} == {k: np.float32(v) for k, v in want.items()}
    text = open(HEADER).read()
    assert f"default {want['sigma_plane']} */" in text and f"for history taps; default {want['reproject_plane']} */" in text


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    lib.uh_denoise_default_params.argtypes, lib.uh_denoise_default_params.restype = [vp], C.c_int
    assert lib.uh_denoise_default_params(None) == 1
    lib.uh_denoise.argtypes, lib.uh_denoise.restype = [vp, vp, vp], C.c_int
    view, good, bad = rr.ViewUniformData(), rr.default_denoise_params(), rr.default_denoise_params()
    bad.iterations = 6
    for p in (good, bad):
        assert lib.uh_denoise(None, C.byref(view), C.byref(p)) == 1
    assert lib.uh_denoise(None, None, None) == 1
    lib.uh_reset_denoise_history.argtypes, lib.uh_reset_denoise_history.restype = [vp], C.c_int
    assert lib.uh_reset_denoise_history(None) == 1
    lib.uh_read_denoised.argtypes, lib.uh_read_denoised.restype = [vp, C.c_int, vp], C.c_int
    buf = (C.c_float * 4)()
    assert lib.uh_read_denoised(None, 0, buf) == 1
    lib.uh_get_denoise_stats.argtypes, lib.uh_get_denoise_stats.restype = [vp, vp], C.c_int
    s = rr.DenoiseStats()
    assert lib.uh_get_denoise_stats(None, C.byref(s)) == 1


def test_python_layer_and_the_oracle_renderer():
    assert (rr.DENOISE_COLOR, rr.DENOISE_OUTPUT, rr.DENOISE_INPUT, rr.DENOISE_TEMPORAL_COLOR, rr.DENOISE_HISTORY, rr.DENOISE_VARIANCE) == tuple(range(6))
    assert rr.Renderer._DENOISE_IMAGES[rr.DENOISE_OUTPUT] == (np.uint8, 4) and rr.Renderer._DENOISE_IMAGES[rr.DENOISE_HISTORY] == (np.float32, 1)
    assert [f[0] for f in rr.DenoiseStats._fields_] == ["pass_ms", "geometry_pixels", "history_pixels", "reserved"]
    o = oa.OracleRenderer(8, 8)
    for call in (lambda: o.denoise(rr.ViewUniformData()), lambda: o.read_denoised(0), o.reset_denoise_history, o.denoise_stats):
        with pytest.raises(NotImplementedError):
            call()

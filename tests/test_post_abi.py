"""CPU: the HDR display chain (UH_HYBRID_POST, UhPostParams, UhPostStats, uh_post_default_params, uh_set_post_params,
uh_reset_post_exposure, uh_get_post_stats, uh_post_image, uh_read_post, uh_post_level_size) at the C ABI, in the C++ host header and in
the Python layer; the level sizes against the restatement, and the header behind them under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import post_reference as pr
import rust_renderer_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "utopian_hip.h")
VERBS = ("uh_post_default_params", "uh_set_post_params", "uh_reset_post_exposure", "uh_get_post_stats", "uh_post_image", "uh_read_post",
         "uh_post_level_size")
FIELDS = ("flags", "tonemap", "bloom_levels", "manual_exposure", "key", "min_exposure", "max_exposure", "adaptation", "low_percentile",
          "high_percentile", "bloom_threshold", "bloom_intensity")
STATS = ("exposure", "target_exposure", "average_luminance", "metered_pixels", "bad_pixels", "levels", "meter_ms", "bloom_ms", "tonemap_ms",
         "renders", "reserved")


def test_header_declares_the_bit_the_verbs_and_the_contract():
    text = open(HEADER).read()
    for s in ("enum { UH_HYBRID_POST = 1u << 16 };", "enum { UH_POST_AUTO_EXPOSURE = 1u << 0, UH_POST_BLOOM = 1u << 1 };",
              "enum { UH_TONEMAP_NONE = 0, UH_TONEMAP_REINHARD = 1, UH_TONEMAP_ACES = 2 };",
              "UH_POST_OUTPUT = 0", "UH_POST_BLOOM_DOWN = 1", "UH_POST_BLOOM_UP = 2", "UH_POST_HISTOGRAM = 3",
              "uint32_t flags, tonemap, bloom_levels;",
              "float manual_exposure, key, min_exposure, max_exposure, adaptation, low_percentile, high_percentile, bloom_threshold, bloom_intensity;",
              "float exposure, target_exposure, average_luminance;", "uint32_t metered_pixels, bad_pixels, levels;",
              "float meter_ms, bloom_ms, tonemap_ms;", "uint32_t renders, reserved[2];",
              "int uh_post_default_params(UhPostParams* out);", "int uh_set_post_params(uh_ctx*, const UhPostParams*);",
              "int uh_reset_post_exposure(uh_ctx*);", "int uh_get_post_stats(uh_ctx*, UhPostStats*);", "int uh_post_image(uh_ctx*, const float* rgba32f);",
              "int uh_read_post(uh_ctx*, int which, int level, void* out);",
              "int uh_post_level_size(uint32_t W, uint32_t H, uint32_t level, uint32_t* w, uint32_t* h);", "UH_HYBRID_FRAME = 0x7f"):
        assert s in text, s
    assert "1u << 9" not in text, "bit 9 stays unused"
    assert "image index must be 0..17" in open(os.path.join(ROOT, "rust-renderer_amd", "csrc", "hybrid_verbs.hip")).read(), "uh_read_hybrid keeps its images"
    for verb in VERBS:
        assert verb.replace("uh_", "uh_mgpu_", 1) not in text, verb
    section = text[text.index("---- HDR display chain"):]
    for s in ("EXTENSION", "PARAMS", "READ-BACK", "RESOURCES", "STREAM ORDER", "ISOLATION", "LIMITS", "NON-FINITE INPUT", "No uh_mgpu_ twin", "present.frag:35-36",
              "bits unchanged", "uh_post_image", "A context that never sets the bit allocates nothing"):
        assert s in section, s
    ordering = text[text.index("---- Stream ordering"):text.index("---- lifetime")]
    for verb in VERBS:
        assert verb in ordering, verb


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_layout_guards_compile_as_c_and_match_ctypes(tmp_path, std):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void) { printf("%zu %zu ", sizeof(UhPostParams), sizeof(UhPostStats));\n' +
                   "".join(f'printf("%zu ", offsetof(UhPostParams, {f}));\n' for f in FIELDS) +
                   "".join(f'printf("%zu ", offsetof(UhPostStats, {f}));\n' for f in STATS) +
                   'printf("%u %u %u %d %d %d %d %d %d %d\\n", (unsigned)UH_HYBRID_POST, (unsigned)UH_POST_AUTO_EXPOSURE, (unsigned)UH_POST_BLOOM, UH_TONEMAP_NONE, '
                   'UH_TONEMAP_REINHARD, UH_TONEMAP_ACES, UH_POST_OUTPUT, UH_POST_BLOOM_DOWN, UH_POST_BLOOM_UP, UH_POST_HISTOGRAM); return 0; }\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = rr.PostParams, rr.PostStats
    assert out == [C.sizeof(P), C.sizeof(S)] + [getattr(P, f).offset for f in FIELDS] + [getattr(S, f).offset for f in STATS] + \
        [rr.HYBRID_POST, rr.POST_AUTO_EXPOSURE, rr.POST_BLOOM, rr.TONEMAP_NONE, rr.TONEMAP_REINHARD, rr.TONEMAP_ACES, rr.POST_OUTPUT, rr.POST_BLOOM_DOWN,
         rr.POST_BLOOM_UP, rr.POST_HISTOGRAM]
    assert out == [48, 48] + list(range(0, 48, 4)) + list(range(0, 44, 4)) + [1 << 16, 1, 2, 0, 1, 2, 0, 1, 2, 3]
    # the guards fire on a packing mismatch
    bad = subprocess.run(["gcc", "-std=c11", "-Dfloat=double", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhPostParams" in bad.stderr and "UhPostStats" in bad.stderr


def test_host_header_has_the_members(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "utopian_host.hpp"\n'
                   "int main() {\n"
                   "   UhPostParams (*a)() = &utopian::Renderer::default_post_params;\n"
                   "   void (utopian::Renderer::*b)(const UhPostParams&) = &utopian::Renderer::set_post_params;\n"
                   "   UhPostStats (utopian::Renderer::*c)() = &utopian::Renderer::post_stats;\n"
                   "   void (utopian::Renderer::*d)() = &utopian::Renderer::reset_post_exposure;\n"
                   "   std::pair<uint32_t, uint32_t> (utopian::Renderer::*e)(uint32_t) const = &utopian::Renderer::post_level_size;\n"
                   "   void (utopian::Renderer::*f)(const float*) = &utopian::Renderer::post_image;\n"
                   "   std::vector<uint8_t> (utopian::Renderer::*g)(int, int) = &utopian::Renderer::read_post;\n"
                   "   return a && b && c && d && e && f && g ? 0 : 1;\n}\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_library_exports_the_verbs_and_no_group_twin():
    lib = rr.load_library()
    for v in VERBS:
        assert hasattr(lib, v), v
        assert not hasattr(lib, v.replace("uh_", "uh_mgpu_", 1)), v


def test_default_params_need_no_gpu_and_match_the_restatement():
    p = rr.post_default_params()
    assert (p.flags, p.tonemap, p.bloom_levels) == (rr.POST_AUTO_EXPOSURE | rr.POST_BLOOM, rr.TONEMAP_ACES, 6)
    assert (p.manual_exposure, p.min_exposure, p.max_exposure, p.low_percentile, p.bloom_threshold) == (1.0, 0.015625, 64.0, 0.5, 1.0)
    assert (p.key, p.adaptation, p.high_percentile, p.bloom_intensity) == tuple(float(np.float32(x)) for x in (0.18, 0.1, 0.95, 0.04))
    want = pr.params()
    assert {f: getattr(p, f) for f in FIELDS} == {k: (float(v) if isinstance(v, np.float32) else v) for k, v in want.items()}
    assert pr.params_of(p) == want
    assert bytes(p) == bytes(rr.Renderer.post_default_params())
    lib = rr.load_library()
    lib.uh_post_default_params.argtypes, lib.uh_post_default_params.restype = [C.c_void_p], C.c_int
    assert lib.uh_post_default_params(None) == 1


def test_level_sizes_match_the_restatement():
    for W, H in pr.SIZES + [(2, 2), (64, 64), (1920, 1080), (2 ** 32 - 1, 3)]:
        for level in range(0, 11):
            want = pr.level_size(W, H, level)
            if want is None:
                with pytest.raises(ValueError, match="no bloom level"):
                    rr.post_level_size(W, H, level)
            else:
                assert rr.post_level_size(W, H, level) == want, (W, H, level)
    with pytest.raises(ValueError):
        rr.post_level_size(0, 4, 0)
    lib = rr.load_library()
    u32, vp = C.c_uint32, C.c_void_p
    lib.uh_post_level_size.argtypes, lib.uh_post_level_size.restype = [u32, u32, u32, vp, vp], C.c_int
    w = u32(77)
    assert lib.uh_post_level_size(4, 4, 1, None, C.byref(w)) == 1 and lib.uh_post_level_size(4, 4, 1, C.byref(w), None) == 1 and w.value == 77
    assert lib.uh_post_level_size(1, 1, 1, C.byref(w), C.byref(w)) == 1 and w.value == 77, "a refused call writes nothing"


def test_null_arguments_are_refused_without_a_device():
    lib = rr.load_library()
    vp = C.c_void_p
    p, s = rr.post_default_params(), rr.PostStats()
    lib.uh_set_post_params.argtypes, lib.uh_set_post_params.restype = [vp, vp], C.c_int
    assert lib.uh_set_post_params(None, C.byref(p)) == 1 and lib.uh_set_post_params(None, None) == 1
    lib.uh_get_post_stats.argtypes, lib.uh_get_post_stats.restype = [vp, vp], C.c_int
    assert lib.uh_get_post_stats(None, C.byref(s)) == 1 and lib.uh_get_post_stats(None, None) == 1
    lib.uh_reset_post_exposure.argtypes, lib.uh_reset_post_exposure.restype = [vp], C.c_int
    assert lib.uh_reset_post_exposure(None) == 1
    lib.uh_post_image.argtypes, lib.uh_post_image.restype = [vp, vp], C.c_int
    assert lib.uh_post_image(None, None) == 1
    lib.uh_read_post.argtypes, lib.uh_read_post.restype = [vp, C.c_int, C.c_int, vp], C.c_int
    assert lib.uh_read_post(None, 0, 0, None) == 1


def test_python_layer():
    assert rr.HYBRID_POST == 1 << 16 and (rr.POST_AUTO_EXPOSURE, rr.POST_BLOOM) == (1, 2)
    assert (rr.TONEMAP_NONE, rr.TONEMAP_REINHARD, rr.TONEMAP_ACES) == (0, 1, 2)
    assert (rr.POST_OUTPUT, rr.POST_BLOOM_DOWN, rr.POST_BLOOM_UP, rr.POST_HISTOGRAM) == (0, 1, 2, 3)
    assert rr.HYBRID_FRAME == 0x7f
    assert rr.HYBRID_POST & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_GBUFFER_RASTER |
                             rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | rr.HYBRID_MOTION | rr.HYBRID_TAA | 1 << 9) == 0
    assert [f[0] for f in rr.PostParams._fields_] == list(FIELDS) and [f[0] for f in rr.PostStats._fields_] == list(STATS)
    for name in ("post_default_params", "set_post_params", "reset_post_exposure", "post_stats", "read_post", "post_level_size", "post_image"):
        assert callable(getattr(rr.Renderer, name)), name
    assert (pr.AUTO_EXPOSURE, pr.BLOOM, pr.NONE, pr.REINHARD, pr.ACES) == (rr.POST_AUTO_EXPOSURE, rr.POST_BLOOM, rr.TONEMAP_NONE, rr.TONEMAP_REINHARD, rr.TONEMAP_ACES)


def test_level_sizes_under_asan_ubsan(tmp_path):
    """csrc/post_levels.h (product code: the sizes behind uh_post_level_size and the pyramid's allocation) under ASan + UBSan: every
    level allocated at the header's size and indexed as the down and up filters index it (tests/cpp/post_levels_check.cpp)"""
    exe = str(tmp_path / "post_levels_check")
    csrc = os.path.join(ROOT, "rust-renderer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-I", csrc, os.path.join(ROOT, "tests", "cpp", "post_levels_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "POST LEVELS CHECK OK" in r.stdout and "FAIL" not in r.stdout

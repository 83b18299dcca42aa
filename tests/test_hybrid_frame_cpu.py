"""CPU: the hybrid graph's final frame (UH_HYBRID_SSAO / DEFERRED / SKY / PRESENT, uh_get_hybrid_frame_stats) at the C ABI and in the
Python layer, and the CPU reference of tests/hybrid_frame_reference.py against known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rust_renderer_amd as rr
from hybrid_util import cast_planes, plane_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
F = np.float32


def test_header_declares_the_final_frame_bits_images_and_verb():
    text = open(HEADER).read()
    for s in ("UH_HYBRID_SSAO = 1u << 3", "UH_HYBRID_DEFERRED = 1u << 4", "UH_HYBRID_SKY = 1u << 5", "UH_HYBRID_PRESENT = 1u << 6",
              "UH_HYBRID_FRAME = 0x7f", "UH_HYBRID_ALL = 7", "UH_HYBRID_SSAO_IMAGE = 6", "UH_HYBRID_DEFERRED_OUTPUT = 7",
              "UH_HYBRID_PRESENT_OUTPUT = 8", "int uh_get_hybrid_frame_stats(uh_ctx* ctx, UhHybridFrameStats* out);"):
        assert s in text, s
    assert text.index("uh_mgpu_set_option(") < text.index("uh_get_hybrid_frame_stats(")
    assert "must clear them" in text, "the header says plainly that the reference's defaults are refused"


@pytest.mark.parametrize("std", ["c11", "c99"])
def test_frame_stats_layout_guard_compiles_as_c_and_matches_ctypes(tmp_path, std):
    src = tmp_path / "f.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n", sizeof(UhHybridFrameStats), offsetof(UhHybridFrameStats, sky_pixels), '
                   'offsetof(UhHybridFrameStats, lights), sizeof(UhHybridStats), UH_HYBRID_SSAO, UH_HYBRID_DEFERRED, UH_HYBRID_SKY, UH_HYBRID_PRESENT, '
                   'UH_HYBRID_FRAME, UH_HYBRID_SSAO_IMAGE, UH_HYBRID_DEFERRED_OUTPUT, UH_HYBRID_PRESENT_OUTPUT); return 0; }\n')
    exe = tmp_path / "f"
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(rr.HybridFrameStats), rr.HybridFrameStats.sky_pixels.offset, rr.HybridFrameStats.lights.offset, C.sizeof(rr.HybridStats),
                   rr.HYBRID_SSAO, rr.HYBRID_DEFERRED, rr.HYBRID_SKY, rr.HYBRID_PRESENT, rr.HYBRID_FRAME, rr.HYBRID_SSAO_IMAGE,
                   rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_PRESENT_OUTPUT] == [48, 28, 32, 48, 8, 16, 32, 64, 127, 6, 7, 8]
    bad = subprocess.run(["gcc", "-std=c11", "-Duint32_t=uint64_t", "-include", "stdint.h", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "b.o")], capture_output=True, text=True)
    assert bad.returncode != 0 and "UhHybridFrameStats" in bad.stderr


def test_library_exports_the_frame_stats_verb_and_rejects_a_null_context():
    lib = rr.load_library()
    assert hasattr(lib, "uh_get_hybrid_frame_stats")
    lib.uh_get_hybrid_frame_stats.argtypes, lib.uh_get_hybrid_frame_stats.restype = [C.c_void_p, C.c_void_p], C.c_int
    s = rr.HybridFrameStats()
    assert lib.uh_get_hybrid_frame_stats(None, C.byref(s)) == 1


def test_python_layer_and_the_oracle_renderer():
    assert rr.HYBRID_FRAME == rr.HYBRID_ALL | rr.HYBRID_SSAO | rr.HYBRID_DEFERRED | rr.HYBRID_SKY | rr.HYBRID_PRESENT
    images = rr.Renderer._HYBRID_IMAGES
    assert images[rr.HYBRID_SSAO_IMAGE] == (np.uint16, 1) and images[rr.HYBRID_DEFERRED_OUTPUT] == (np.float32, 4)
    assert images[rr.HYBRID_PRESENT_OUTPUT] == (np.uint8, 4)
    o = oa.OracleRenderer(8, 8)
    with pytest.raises(NotImplementedError):
        o.hybrid_frame_stats()


# ---- known answers of the reference ---------------------------------------------------------------------------------------------
W, H = 48, 36


def test_ssao_of_a_flat_plane_facing_the_camera_is_exactly_one():
    view = plane_view((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    pos, nrm = cast_planes(view, [((0.0, 0.0, -3.0), np.array([0.0, 0.0, 1.0]))], W, H)
    assert (pos[..., 3] == 1).all()
    assert (fr.ssao(pos, nrm, view) == 65535).all(), "every kernel sample has z > 0: in front of the plane"


def test_ssao_darkens_an_inside_corner_and_only_near_it():
    view = plane_view((0.0, 0.2, 0.0), (0.0, -0.6, -2.0), W, H)
    pos, nrm = cast_planes(view, [((0.0, -0.5, 0.0), np.array([0.0, 1.0, 0.0])), ((0.0, 0.0, -2.0), np.array([0.0, 0.0, 1.0]))], W, H)
    occ = fr.ssao(pos, nrm, view)
    crease = np.abs(pos[..., 1] + 0.5) + np.abs(pos[..., 2] + 2.0) < 0.05  # G-buffer texels at the corner
    far = (np.abs(pos[..., 1] + 0.5) + np.abs(pos[..., 2] + 2.0) > 0.6) & (pos[..., 3] == 1)
    assert crease.any() and far.any()
    occ_of_gbuffer = occ[::-1]  # ssao texel (x, y) belongs to G-buffer texel (x, H-1-y)
    assert occ_of_gbuffer[crease].max() < 65535 and occ_of_gbuffer[crease].mean() < 60000
    assert (occ_of_gbuffer[far] == 65535).all()


def test_one_sunlit_lambertian_pixel_is_the_closed_form_surface_shading():
    view = plane_view((0.0, 5.0, 0.0), (0.0, 0.0, -1.0), W, H)
    view.eye_pos[:] = (0.0, 5.0, 0.0)
    view.sun_dir[:] = (0.0, 1.0, 0.0)
    view.raytracing_supported = view.ssao_enabled = 0
    view.num_lights = 0
    g = dict(position=np.array([[[0.0, 0.0, 0.0, 1.0]]], np.float32), normal=np.array([[[0.0, 1.0, 0.0, 1.0]]], np.float32),
             albedo=np.array([[[255, 255, 255, 255]]], np.uint8), pbr=np.array([[[0.0, 1.0, 1.0, 0.0]]], np.float32))
    meshes = [dict(metallic=F(1.0), roughness=F(1.0), base_color=np.ones(3, np.float32), type=0.0)]
    got = fr.deferred(g, np.zeros((1, 1), np.uint8), np.zeros((1, 1, 4), np.uint8), np.zeros((1, 1), np.uint16), view, meshes, [])
    # N = V = L = H: NDF = 1 / pi (roughness 1), G = 1, F = F0 = 0.04, kD = 0.96
    pi = float(np.float32(3.14159265359))
    spec = (1.0 / pi) * 0.04 / (4.0 + 0.0001)
    want = 0.03 + (0.96 / pi + spec)
    assert np.allclose(got[0, 0, :3], want, rtol=2e-6, atol=0) and got[0, 0, 3] == 1.0


def test_a_point_light_below_the_horizon_adds_nothing_and_one_above_adds_its_share():
    view = plane_view((0.0, 5.0, 0.0), (0.0, 0.0, -1.0), W, H)
    view.eye_pos[:] = (0.0, 5.0, 0.0)
    view.sun_dir[:] = (0.6, -0.8, 0.0)  # the sun below the horizon: NdotL = 0 (not opposite V, where H = normalize(0) is NaN)
    view.raytracing_supported = view.ssao_enabled = 0
    g = dict(position=np.array([[[0.0, 0.0, 0.0, 1.0]]], np.float32), normal=np.array([[[0.0, 1.0, 0.0, 1.0]]], np.float32),
             albedo=np.array([[[255, 255, 255, 255]]], np.uint8), pbr=np.array([[[0.0, 1.0, 1.0, 0.0]]], np.float32))
    meshes = [dict(metallic=F(1.0), roughness=F(1.0), base_color=np.ones(3, np.float32), type=0.0)]
    args = (np.zeros((1, 1), np.uint8), np.zeros((1, 1, 4), np.uint8), np.zeros((1, 1), np.uint16))
    below, above = rr.make_light((0.5, -2.0, 0.0)), rr.make_light((0.0, 2.0, 0.0))
    view.num_lights = 1
    assert np.array_equal(fr.deferred(g, *args, view, meshes, [below])[0, 0, :3], np.full(3, F(0.03)))
    got = fr.deferred(g, *args, view, meshes, [above])[0, 0, :3]
    pi = float(np.float32(3.14159265359))
    att = 1.0 / (0.0 + 0.0 * 2.0 + 0.1 * 4.0)  # make_light: attenuation (0, 0, 0.1)
    want = 0.03 + (0.96 / pi + (1.0 / pi) * 0.04 / 4.0001) * att
    assert np.allclose(got, want, rtol=2e-6, atol=0)


def test_a_constant_image_passes_fxaa_unchanged():
    img = np.zeros((H, W, 4), np.float32)
    img[..., :3] = (0.8, 0.3, 0.05)
    assert np.array_equal(fr.fxaa(img), img[..., :3])
    out = fr.present(img)
    want = hr.unorm8(fr.linear_to_srgb(np.array([0.05, 0.3, 0.8], np.float32)))  # B, G, R
    assert (out[..., :3] == want).all() and (out[..., 3] == 255).all()


def test_fxaa_softens_a_hard_edge_and_only_at_the_edge():
    img = np.zeros((H, W, 4), np.float32)
    img[:, W // 2:, :3] = 1.0
    out = fr.fxaa(img)
    changed = np.any(out != img[..., :3], axis=-1)
    assert changed.any() and set(np.nonzero(changed)[1]) <= {W // 2 - 1, W // 2}


def test_linear_to_srgb_matches_the_formula():
    c = np.concatenate([np.linspace(0.0, 0.004, 101), np.linspace(0.004, 1.0, 2001), [1.5, 0.0031308]]).astype(np.float32)
    x = c.astype(np.float64)
    want = np.where(c < np.float32(0.0031308), x * 12.92, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    assert np.abs(fr.linear_to_srgb(c) - want).max() < 2e-7

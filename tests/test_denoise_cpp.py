"""The denoiser through the C++ host mirror (include/utopian_host.hpp, tests/cpp/denoise_host.cpp): it builds and links here; on the GPU
its six images after two calls equal those of the ctypes path on the same scene bytes."""
import os
import subprocess

import numpy as np
import pytest

import rust_renderer_amd as rr
from hybrid_util import CPP_H, CPP_W, ROOT, cpp_scene, cpp_view, write_blob


def build(tmp_path):
    exe = str(tmp_path / "denoise_host")
    libdir = os.path.dirname(rr.api.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "denoise_host.cpp"),
                    "-o", exe, "-L", libdir, "-lutopian_hip", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def denoise_view():
    v = cpp_view()
    v.samples_per_frame = v.total_samples = 1
    v.use_ris_light_sampling = 0
    v.time = 0.25
    proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
    view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
    v.prev_frame_projection_view[:] = tuple((proj @ view).astype(np.float32).T.reshape(-1))
    return v


def test_cpp_denoise_host_builds_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_cpp_denoised_images_equal_the_ctypes_images(tmp_path):
    meshes, v = cpp_scene(), denoise_view()
    blob, out = tmp_path / "scene.blob", tmp_path / "out.bin"
    write_blob(blob, meshes, v)
    res = subprocess.run([build(tmp_path), str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(out, dtype=np.uint8)
    r = rr.Renderer(CPP_W, CPP_H)
    white = r.default_diffuse_map()
    for vert, idx, kind, base in meshes:
        r.add_mesh(vert, idx, rr.make_material(kind, 0.0, base, diffuse_map=white))
    r.initialize_raytracing()
    for _ in range(2):
        r.render_frame(v, rr.PASS_REFERENCE_PT)
        r.render_hybrid(v, rr.HYBRID_GBUFFER)
        r.denoise(v)
        v.time += 0.125
    at = 0
    for which in range(6):
        mine = r.read_denoised(which).view(np.uint8).reshape(-1)
        assert np.array_equal(got[at : at + mine.size], mine), which
        at += mine.size
    assert at == got.size
    s = r.denoise_stats()
    assert f"geometry {s.geometry_pixels} history {s.history_pixels}" in res.stdout and s.history_pixels > 0
    assert r.read_denoised(rr.DENOISE_HISTORY).max() == 2

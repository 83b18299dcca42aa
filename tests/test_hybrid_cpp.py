"""The hybrid passes through the C++ host mirror (include/utopian_host.hpp, tests/cpp/hybrid_host.cpp): it builds and links here; on the
GPU its six images equal those of the ctypes path on the same scene bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rust_renderer_amd as rr
from rust_renderer_amd.scenes import icosphere, quad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64


def build_cpp(tmp_path):
    exe = str(tmp_path / "hybrid_host")
    libdir = os.path.dirname(rr.api.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "hybrid_host.cpp"),
                    "-o", exe, "-L", libdir, "-lutopian_hip", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def scene():
    """(vertices, indices, material type, base colour) per mesh, identity transforms: a metal floor, a Lambertian sphere, a metal sphere"""
    fv, fi = quad((-5.0, 0.0, 5.0), (10.0, 0.0, 0.0), (0.0, 0.0, -10.0), nu=4, nv=4)
    sv, si = icosphere(2)
    sv2 = sv.copy()
    sv["pos"][:, :3] = sv["pos"][:, :3] * 0.8 + np.array([-1.0, 0.8, 0.0], np.float32)
    sv2["pos"][:, :3] = sv2["pos"][:, :3] * 0.6 + np.array([1.0, 0.6, 0.5], np.float32)
    return [(fv, fi, rr.METAL, (0.9, 0.9, 0.9, 1.0)), (sv, si, rr.LAMBERTIAN, (0.8, 0.3, 0.2, 1.0)), (sv2, si, rr.METAL, (1.0, 1.0, 1.0, 1.0))]


def view():
    cam = rr.camera.Camera((0.0, 2.0, 5.0), (0.0, 0.7, 0.0), 60.0, W / H, 0.01, 1000.0)
    v = rr.default_view(cam, W, H)
    v.ibl_enabled = 0
    return v


def write_blob(path, meshes, v):
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x44594855, W, H))
        f.write(bytes(v))
        f.write(struct.pack("<I", len(meshes)))
        for vert, idx, kind, base in meshes:
            f.write(struct.pack("<III4f", len(vert), len(idx), kind, *base))
            f.write(np.ascontiguousarray(vert).tobytes())
            f.write(np.ascontiguousarray(idx, dtype=np.uint32).tobytes())


def test_cpp_hybrid_host_builds_and_links(tmp_path):
    assert os.path.exists(build_cpp(tmp_path))


@pytest.mark.gpu
def test_cpp_hybrid_images_equal_the_ctypes_images(tmp_path):
    exe = build_cpp(tmp_path)
    meshes, v = scene(), view()
    blob, out = tmp_path / "scene.blob", tmp_path / "out.bin"
    write_blob(blob, meshes, v)
    res = subprocess.run([exe, str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    r = rr.Renderer(W, H)
    white = r.default_diffuse_map()
    for vert, idx, kind, base in meshes:
        r.add_mesh(vert, idx, rr.make_material(kind, 0.0, base, diffuse_map=white))
    r.initialize_raytracing()
    r.render_hybrid(v, rr.HYBRID_GBUFFER)
    r.render_hybrid(v)
    blob_out = np.fromfile(out, dtype=np.uint8)
    at = 0
    for which in range(6):
        mine = r.read_hybrid(which).view(np.uint8).reshape(-1)
        assert np.array_equal(blob_out[at : at + mine.size], mine), which
        at += mine.size
    assert at == blob_out.size
    s = r.hybrid_stats()
    assert f"rays {s.rays[0]} {s.rays[1]} {s.rays[2]} metal {s.reflection_pixels}" in res.stdout and s.reflection_pixels > 0

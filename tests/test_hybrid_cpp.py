"""The hybrid passes through the C++ host mirror (include/utopian_host.hpp, tests/cpp/hybrid_host.cpp in its passes mode): it builds
and links here; on the GPU its six images equal those of the ctypes path on the same scene bytes."""
import os

import numpy as np
import pytest

import rust_renderer_amd as rr
from hybrid_util import build_cpp, cpp_scene, cpp_view, run_cpp


def test_cpp_hybrid_host_builds_and_links(tmp_path):
    assert os.path.exists(build_cpp(tmp_path))


@pytest.mark.gpu
def test_cpp_hybrid_images_equal_the_ctypes_images(tmp_path):
    meshes, v = cpp_scene(), cpp_view()
    res, blob_out, r = run_cpp(tmp_path, "passes", meshes, v)
    r.render_hybrid(v, rr.HYBRID_GBUFFER)
    r.render_hybrid(v)
    at = 0
    for which in range(6):
        mine = r.read_hybrid(which).view(np.uint8).reshape(-1)
        assert np.array_equal(blob_out[at : at + mine.size], mine), which
        at += mine.size
    assert at == blob_out.size
    s = r.hybrid_stats()
    assert f"rays {s.rays[0]} {s.rays[1]} {s.rays[2]} metal {s.reflection_pixels}" in res.stdout and s.reflection_pixels > 0

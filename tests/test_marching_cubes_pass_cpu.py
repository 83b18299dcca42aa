"""CPU: the marching-cubes pass's restatement (tests/marching_cubes_pass_reference.py) against known answers - the extraction against the
oracle, the seeded depth test's tie rule, the depth buffer's clipping - and the pass's public constants and stats layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forward_reference as fw
import marching_cubes_pass_reference as mr
import oracle_api as oa
import rust_renderer_amd as rr
from hybrid_util import ROOT
from rust_renderer_amd.scenes import Scene

F = np.float32
W, H = 16, 12


@pytest.mark.parametrize("t", [0.0, 5.0])
def test_extraction_equals_the_oracle(t):
    _, table = oa.mc_reference_tables()
    pos, nrm = mr.extract(t, table)
    ref = oa.marching_cubes(32, 0.0, 32.0, t)
    assert len(pos) == ref["triangles"] > 1000
    assert np.array_equal(pos.view(np.uint32), ref["positions"].view(np.uint32)), "positions bit for bit, in draw order"
    unit = np.abs(np.linalg.norm(nrm.astype(np.float64), axis=-1) - 1.0) < 1e-5
    assert np.isfinite(nrm).all() and unit.mean() > 0.99  # a vertex where the central differences cancel keeps a short normal


def test_extraction_normals_follow_the_density():
    _, table = oa.mc_reference_tables()
    pos, nrm = mr.extract(5.0, table)
    r = mr.sphere_radius(5.0)
    # generateNormal points out of the solid: a small step along it lowers the density
    p = pos.reshape(-1, 3)[::97]
    n = nrm.reshape(-1, 3)[::97]
    d_out = mr.density(*(p + F(0.05) * n).T, r)
    d_in = mr.density(*(p - F(0.05) * n).T, r)
    assert (d_out < d_in).mean() > 0.95


def _view(eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0)):
    cam = rr.camera.Camera(eye, target, 60.0, W / H, 0.1, 100.0)
    v = Scene("t", [], [], cam, {}).make_view(W, H)
    v.shadows_enabled = 0
    return v


def _material():
    return dict(diffuse_map=0, normal_map=0, metallic_roughness_map=0, occlusion_map=0, base_color=np.ones(3, F))


def _triangle_at(z):
    """one triangle at world depth z covering the centre of the frame, normals towards the camera"""
    p = np.array([[[-1.0, -1.0, z], [1.0, -1.0, z], [0.0, 1.0, z]]], F)
    n = np.tile(np.array([0.0, 0.0, 1.0], F), (1, 3, 1))
    return mr.pass_mesh(p, n, _material())


def _gbuffer_at(z):
    """a G-buffer whose every pixel sees a surface at world depth z"""
    pos = np.zeros((H, W, 4), F)
    pos[..., 2], pos[..., 3] = z, 1.0
    return pos


def test_a_fragment_at_the_seeded_depth_survives():
    view = _view()
    mesh = _triangle_at(0.0)
    recs = fw.records_for([mesh], view, W, H)
    depth0, vis0, _ = fw.resolve(recs, W, H)
    covered = vis0 != fw.NONE
    assert covered.sum() > 10
    # the G-buffer's depth where the triangle covers the pixel: exactly the triangle's depth there (a plane z = 0 seen head on)
    seed = np.where(covered, depth0, F(1.0)).astype(F)
    depth, vis, rec = mr.resolve_seeded(recs, seed, W, H)
    assert np.array_equal(vis, vis0) and np.array_equal(depth.view(np.uint32), seed.view(np.uint32)), "LESS_OR_EQUAL: the seed loses ties"
    nearer = np.where(covered, np.nextafter(depth0, F(0.0)), F(1.0)).astype(F)
    _, vis, rec = mr.resolve_seeded(recs, nearer, W, H)
    assert (vis == fw.NONE).all() and (rec < 0).all(), "a nearer G-buffer hides it"


def test_the_pass_draws_in_front_and_hides_behind():
    view = _view()
    mesh = _triangle_at(0.0)
    deferred = np.full((H, W, 4), 0.25, F)
    textures = [np.full((1, 1, 4), 200, np.uint8)]
    front = mr.marching_cubes_pass(mesh, textures, view, [], _gbuffer_at(-1.0), deferred)
    covered = front["visibility"] != fw.NONE
    assert covered.sum() > 10
    assert (front["output"][covered, 3] == 1.0).all() and np.array_equal(front["output"][~covered], deferred[~covered])
    behind = mr.marching_cubes_pass(mesh, textures, view, [], _gbuffer_at(1.0), deferred)
    assert (behind["visibility"] == fw.NONE).all() and np.array_equal(behind["output"], deferred)
    assert np.array_equal(behind["depth"], behind["seed"])


def test_depth_seed_clips_to_the_depth_range():
    view = _view()  # near 0.1, far 100, the camera at z = 3 looking down -z
    pos = np.zeros((1, 4, 4), F)
    pos[0, :, 3] = 1.0
    pos[0, 0, 2] = 0.0     # inside: 0 < d < 1
    pos[0, 1, 2] = -500.0  # beyond the far plane: d > 1
    pos[0, 2, 2] = 2.95    # in front of the near plane: d < 0
    pos[0, 3, 2] = 10.0    # behind the camera: c.w < 0
    d = mr.depth_seed(pos, view)[0]
    assert 0.0 < d[0] < 1.0
    assert d[1] == 1.0 and d[2] == 1.0 and d[3] == 1.0
    miss = np.zeros((1, 1, 4), F)
    assert mr.depth_seed(miss, view)[0, 0] == 1.0, "a miss is 1.0"


def test_python_constants():
    assert rr.HYBRID_MARCHING_CUBES == 1 << 10 and rr.HYBRID_FRAME == 0x7F
    assert rr.HYBRID_DEPTH == 9 and rr.HYBRID_MARCHING_CUBES_VISIBILITY == 10 and rr.MARCHING_CUBES_NONE == 0xFFFFFFFF
    assert not rr.HYBRID_MARCHING_CUBES & (rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS | (1 << 9))
    s = rr.MarchingCubesStats
    assert C.sizeof(s) == 32 and s.triangles.offset == 8 and s.pieces.offset == 12 and s.covered_pixels.offset == 16
    assert s.lights.offset == 20 and s.time.offset == 24


def test_library_exports_the_stats_verb():
    lib = rr.load_library()
    assert hasattr(lib, "uh_get_marching_cubes_stats")


def test_layout_guard_compiles_and_matches_ctypes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "utopian_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %d %d %d\\n\", sizeof(UhMarchingCubesStats),"
                   " offsetof(UhMarchingCubesStats, triangles), offsetof(UhMarchingCubesStats, pieces),"
                   " offsetof(UhMarchingCubesStats, covered_pixels), offsetof(UhMarchingCubesStats, lights),"
                   " offsetof(UhMarchingCubesStats, time), UH_HYBRID_MARCHING_CUBES, UH_HYBRID_DEPTH, UH_HYBRID_MARCHING_CUBES_VISIBILITY);"
                   " return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    s = rr.MarchingCubesStats
    assert [int(x) for x in out] == [C.sizeof(s), s.triangles.offset, s.pieces.offset, s.covered_pixels.offset, s.lights.offset, s.time.offset,
                                     1 << 10, 9, 10]

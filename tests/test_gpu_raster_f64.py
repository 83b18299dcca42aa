"""GPU: the four rasterised passes on the device against the independent float64 rasteriser of tests/raster_f64.py, through no
restatement: uh_render_forward's depth and visibility, the rasterised G-buffer's depth, visibility and world position, the four shadow
cascades and the marching-cubes pass's depth and visibility, under the decision rule, on the cases and with the absolute terms of
tests/raster_f64_cases.py. The device equals the restatements bit for bit (test_gpu_forward.py and its siblings), so a failure
here that test_raster_f64_cpu.py does not show means kernel and restatement differ at a case those tests do not draw."""
import numpy as np
import pytest

import raster_f64 as rf
import rust_renderer_amd as rr
from rust_renderer_amd.types import VERTEX_DTYPE
from raster_f64_cases import B_ULPS, CASES, DEPTH_ULPS, MC_H, MC_TIME, MC_W, SHADOW_CASES, SHADOW_SIZE, case_view, mc_case, mc_checks, prepared, recorded, report, \
    shadow_caps, shadow_checks, shadow_truths

pytestmark = pytest.mark.gpu
RASTER = rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER


def _device(case):
    gpu = rr.Renderer(case["W"], case["H"])
    case["scene"].upload(gpu)
    return gpu


@pytest.mark.parametrize("name", list(CASES))
def test_forward_pass(name):
    p = prepared(name)
    case, five = p["case"], p["five"]
    gpu = _device(case)
    gpu.render_forward(p["view"], rr.FORWARD_PASS)
    rf.check_caps(five, case["exempt"])
    rf.check_visibility(five, gpu.read_forward(rr.FORWARD_VISIBILITY), case["excused"])
    dz = rf.check_depth(five, gpu.read_forward(rr.FORWARD_DEPTH), case["depth_ulps"])
    report(name, "forward, device", five, depth_excess_ulps=dz)


@pytest.mark.parametrize("name", list(CASES))
def test_rasterised_gbuffer(name):
    p = prepared(name)
    case, five = p["case"], p["five"]
    gpu = _device(case)
    gpu.render_hybrid(p["view"], RASTER)
    vis = gpu.read_hybrid(rr.HYBRID_GBUFFER_VISIBILITY)
    rf.check_caps(five, case["exempt"])
    rf.check_visibility(five, vis, case["excused"])
    dz = rf.check_depth(five, gpu.read_hybrid(rr.HYBRID_GBUFFER_DEPTH), case["depth_ulps"])
    pos = gpu.read_hybrid(rr.HYBRID_POSITION).reshape(-1, 4)
    covered = vis.reshape(-1) != rf.NONE
    assert np.array_equal(pos[:, 3] == 1.0, covered), "w marks the covered pixels"
    pix = np.nonzero(covered)[0]
    rf.check_positions(five, p["meshes"], pix, pos[pix, :3], B_ULPS)
    report(name, "gbuffer, device", five, depth_excess_ulps=dz)


@pytest.mark.parametrize("name", SHADOW_CASES)
def test_shadow_maps(name):
    p = prepared(name)
    case, view = p["case"], p["view"]
    gpu = _device(case)
    gpu.set_option("shadow_map_size", SHADOW_SIZE)
    params = rr.shadow_cascades(case["scene"].camera, view.sun_dir[:])
    gpu.set_shadowmap_params(params)
    v = case_view(case)
    v.shadows_enabled = 1
    gpu.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    fives = shadow_truths(case, p["meshes"], params)
    shadow_caps(name, fives)
    dz = max(shadow_checks(fives[c], gpu.read_shadow_map(c), DEPTH_ULPS) for c in range(4))
    print(f"{name} [shadow maps, device]: depth_excess_ulps={dz:.2f}")


def _flat_mesh(positions):
    """a triangle list (T, 3, 3) as raster_f64 reads a mesh: vertex 3 t + k, the identity for a world matrix"""
    v = np.zeros(3 * len(positions), VERTEX_DTYPE)
    v["pos"][:, :3], v["pos"][:, 3] = positions.reshape(-1, 3), 1.0
    return dict(vertices=v, indices=np.arange(len(v), dtype=np.uint32), world=rr.identity3x4())


def test_marching_cubes_pass():
    case = mc_case()
    view = case_view(case)
    gpu = _device(case)
    gpu.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MARCHING_CUBES)
    seed = gpu.read_hybrid(rr.HYBRID_GBUFFER_DEPTH)  # the pass tests against the rasterised G-buffer's own depth buffer
    depth, vis = gpu.read_hybrid(rr.HYBRID_DEPTH), gpu.read_hybrid(rr.HYBRID_MARCHING_CUBES_VISIBILITY)
    other = rr.Renderer(8, 8)  # the pass's triangles: those of uh_add_isosurface_mesh on the reference's grid, in extraction order
    index, tris = other.add_isosurface_mesh(32, 0.0, 32.0, MC_TIME)
    vtx, idx = other.read_mesh(index)
    assert len(idx) == 3 * tris == 3 * gpu.marching_cubes_stats().triangles
    mesh = _flat_mesh(vtx[idx]["pos"][:, :3].reshape(-1, 3, 3))
    five = rf.five_points(rf.view_matrices(view, [mesh]), [mesh], MC_W, MC_H, seed=seed)
    rf.check_caps(five)
    assert (five.decided & (five.winner < 0) & (seed < 1.0)).sum() > 20, "the occluders hide part of the isosurface"
    dz = mc_checks(five, vis, depth, seed, DEPTH_ULPS)
    report("marching_cubes", "seeded, device", five, depth_excess_ulps=dz)
    # and the depth buffer it was seeded by, against the occluders' truth
    meshes = recorded(case)
    occluders = rf.five_points(rf.view_matrices(view, meshes), meshes, MC_W, MC_H)
    rf.check_visibility(occluders, gpu.read_hybrid(rr.HYBRID_GBUFFER_VISIBILITY))
    rf.check_depth(occluders, seed, DEPTH_ULPS)

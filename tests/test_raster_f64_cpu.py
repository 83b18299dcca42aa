"""CPU: the numpy restatements of the four rasterised passes (forward_reference, gbuffer_raster_reference, marching_cubes_pass_reference,
shadow_map_reference - the contract of DESIGN.md section 2 the kernels are held to bit for bit) against the independent float64
rasteriser of tests/raster_f64.py, under its decision rule, on the cases and with the absolute terms of tests/raster_f64_cases.py, which
also says where each term was measured. A failure here means the contract itself is wrong.

Shown to bite on a scratch copy of forward_reference.py: a near-plane crossing computed from `cur` towards `nxt` leaves a crack at
spokes_behind_the_eye (a surely covered pixel empty); the per-fragment test `zz > 0` empties the 272 surely covered pixels of
near_plane_tie; dropping the last fan triangle of a guard-band piece empties 1,612 decided pixels of huge_floor_fan_in_view and 169 of
spokes_behind_the_eye. Each is caught by the one or two cases built for it, `zz > 0` only by the quad lying exactly in the near plane."""
import numpy as np
import pytest

import forward_reference as fw
import gbuffer_raster_reference as gr
import marching_cubes_pass_reference as mr
import oracle_api as oa
import raster_f64 as rf
import rust_renderer_amd as rr
import shadow_map_reference as sr
from raster_f64_cases import B_ULPS, CASES, DEPTH_ULPS, MC_H, MC_TIME, MC_W, SHADOW_CASES, SHADOW_SIZE, case_view, mc_case, mc_checks, prepared, recorded, \
    report, shadow_caps, shadow_checks, shadow_truths
from rust_renderer_amd.types import VERTEX_DTYPE

TEXTURES = []  # no case adds a texture: every map index reads white


# ---- the forward pass and the rasterised G-buffer -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_forward_restatement(name):
    p = prepared(name)
    case, meshes, view, five = p["case"], p["meshes"], p["view"], p["five"]
    W, H = case["W"], case["H"]
    ref = fw.forward(meshes, TEXTURES, view, [], W, H)
    rf.check_caps(five, case["exempt"])
    rf.check_visibility(five, ref["visibility"], case["excused"])
    dz = rf.check_depth(five, ref["depth"], case["depth_ulps"])
    _, _, rec = fw.resolve(ref["records"], W, H)
    pix, b = fw.barycentrics(ref["records"], rec, W, H)
    assert np.array_equal(pix, ref["pixels"])
    db = rf.check_barycentrics(five, pix, b, B_ULPS)  # a record's B rows carry the original triangle's vertices through clip and swap
    rf.check_positions(five, meshes, pix, ref["position"], B_ULPS)
    report(name, "forward", five, depth_excess_ulps=dz, b_excess_ulps=db)


@pytest.mark.parametrize("name", list(CASES))
def test_gbuffer_raster_restatement(name):
    p = prepared(name)
    case, meshes, view, five = p["case"], p["meshes"], p["view"], p["five"]
    W, H = case["W"], case["H"]
    ref = gr.gbuffer_raster(meshes, TEXTURES, view, W, H)
    rf.check_caps(five, case["exempt"])
    rf.check_visibility(five, ref["visibility"], case["excused"])
    dz = rf.check_depth(five, ref["depth"], case["depth_ulps"])
    _, _, rec = fw.resolve(ref["records"], W, H)
    pix, b = fw.barycentrics(ref["records"], rec, W, H)
    db = rf.check_barycentrics(five, pix, b, B_ULPS)
    pos = ref["position"].reshape(-1, 4)
    assert np.array_equal(pos[:, 3] == 1.0, (ref["visibility"] != gr.NONE).reshape(-1))
    rf.check_positions(five, meshes, pix, pos[pix, :3], B_ULPS)
    report(name, "gbuffer", five, depth_excess_ulps=dz, b_excess_ulps=db)


def test_inside_the_cube_every_pixel_is_surely_covered():
    assert prepared("inside_cube")["five"].covered.all()


def test_the_quad_in_the_near_plane_is_surely_covered():
    five = prepared("near_plane_tie")["five"]
    mine = five.covered & (five.winner == 0)
    assert mine.sum() > 100 and (five.d[:, mine] == 0.0).all() and not five.decided[mine].any()


def test_fan_and_diagonal_leave_centres_undecided_but_covered():
    five = prepared("fan_and_diagonal")["five"]
    on_edge = five.covered & ~five.decided
    assert on_edge[23, 16], "the fan's centre vertex: pixel (16, 23)"
    assert all(on_edge[33 - k, 36 + k] for k in range(1, 20)), "the quad's diagonal"


# ---- the shadow maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHADOW_CASES)
def test_shadow_map_restatement(name):
    p = prepared(name)
    case, meshes = p["case"], p["meshes"]
    params = rr.shadow_cascades(case["scene"].camera, p["view"].sun_dir[:])
    maps = sr.shadow_maps(meshes, params, SHADOW_SIZE)
    fives = shadow_truths(case, meshes, params)
    shadow_caps(name, fives)
    dz = max(shadow_checks(fives[c], maps[c], DEPTH_ULPS) for c in range(4))
    print(f"{name} [shadow maps]: depth_excess_ulps={dz:.2f}")


# ---- the marching-cubes pass ----------------------------------------------------------------------------------------------------
def test_marching_cubes_pass_restatement():
    case = mc_case()
    meshes = recorded(case)
    view = case_view(case)
    pos, nrm = mr.extract(MC_TIME, oa.mc_reference_tables()[1])
    mesh = mr.pass_mesh(pos, nrm, meshes[0])
    seed = fw.resolve(fw.records_for(meshes, view, MC_W, MC_H), MC_W, MC_H)[0]
    depth, vis, _ = mr.resolve_seeded(fw.records_for([mesh], view, MC_W, MC_H), seed, MC_W, MC_H)
    five = rf.five_points(rf.view_matrices(view, [mesh]), [mesh], MC_W, MC_H, seed=seed)
    rf.check_caps(five)
    assert (five.decided & (five.winner < 0) & (seed < 1.0)).sum() > 20, "the occluders hide part of the isosurface"
    dz = mc_checks(five, vis, depth, seed, DEPTH_ULPS)
    report("marching_cubes", "seeded", five, depth_excess_ulps=dz)


# ---- the truth's own known answers ------------------------------------------------------------------------------------------------
def _mesh(pos, indices):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["pos"][:, :3], v["pos"][:, 3] = pos, 1.0
    return dict(vertices=v, indices=np.asarray(indices, np.uint32), world=rr.identity3x4())


def _rays(eye, target, fov, W, H):
    """float64 pinhole rays through the pixel centres from the camera's definition alone (no matrix): eye, unit directions (H, W, 3)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, [0.0, 1.0, 0.0])
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    t = np.tan(np.radians(fov) / 2.0)
    x = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * t * W / H
    y = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * t
    X, Y = np.meshgrid(x, y)
    d = f + X[..., None] * s + Y[..., None] * u
    return eye, d / np.linalg.norm(d, axis=-1, keepdims=True), f


def test_truth_on_a_head_on_quad():
    W, H, D, fov, near, far = 48, 40, 3.0, 60.0, 0.1, 100.0
    ax, ay = 1.03, 0.71
    view = rr.default_view(rr.camera.Camera((0.0, 0.0, D), (0.0, 0.0, 0.0), fov, W / H, near, far), W, H)
    m = _mesh([(-ax, -ay, 0.0), (ax, -ay, 0.0), (ax, ay, 0.0), (-ax, ay, 0.0)], [0, 1, 2, 0, 2, 3])
    t = rf.truth(rf.view_matrices(view, [m]), [m], W, H)
    # the pixel centre's point in the plane z = 0: (x_ndc aspect, y_ndc) D tan(fov / 2)
    k = D * np.tan(np.radians(fov) / 2.0)
    x = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * k * W / H
    y = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * k
    X, Y = np.meshgrid(x, y)
    assert min(np.abs(np.abs(X) - ax).min(), np.abs(np.abs(Y) - ay).min()) > 1e-3, "no centre next to an edge"
    inside = (np.abs(X) < ax) & (np.abs(Y) < ay)
    assert 300 < inside.sum() < W * H
    assert np.array_equal(t["winner"] >= 0, inside)
    # x + y > 0 is triangle 0's side of the diagonal scaled: the diagonal runs from (-ax, -ay) to (ax, ay)
    lower = (Y * ax < X * ay)
    assert np.array_equal(t["winner"][inside], np.where(lower, 0, 1)[inside])
    want = far * (D - near) / ((far - near) * D)
    assert np.abs(t["d"][inside] - want).max() < 1e-6 and np.isinf(t["d"][~inside]).all() and np.isinf(t["runner"]).all()
    assert np.abs(t["b"][inside].sum(-1) - 1.0).max() < 1e-12


def test_truth_uv_on_a_steep_receding_plane():
    W, H, L = 128, 128, 8.0
    eye, target, fov, near, far = (0.0, 1.5, 0.0), (0.0, 0.0, -3.0), 60.0, 0.1, 50.0
    view = rr.default_view(rr.camera.Camera(eye, target, fov, W / H, near, far), W, H)
    pos = [(-2.0, 0.0, -0.5), (2.0, 0.0, -0.5), (2.0, 0.0, -0.5 - L), (-2.0, 0.0, -0.5 - L)]
    uv = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    idx = np.array([0, 1, 2, 0, 2, 3])
    m = _mesh(pos, idx)
    t = rf.truth(rf.view_matrices(view, [m]), [m], W, H)
    hit = t["winner"] >= 0
    assert hit.sum() > 1500
    got = (uv[idx.reshape(-1, 3)[t["winner"][hit]]] * t["b"][hit][..., None]).sum(1)
    o, d, f = _rays(eye, target, fov, W, H)
    s = -o[1] / d[hit][:, 1]
    p = o + s[:, None] * d[hit]
    want = np.stack([(p[:, 0] + 2.0) / 4.0, (-0.5 - p[:, 2]) / L], -1)
    assert np.abs(got - want).max() < 1e-5, "perspective-correct: the float32 matrices' rounding only"
    z = (p - o) @ f
    assert np.abs(t["d"][hit] - far * (z - near) / ((far - near) * z)).max() < 1e-5
    # the points of the plane outside the quad, and the sky, are empty
    U = (o[0] + (-o[1] / d[..., 1])[..., None] * d[..., 0:1])[..., 0]
    assert not t["winner"][(d[..., 1] >= 0)].max() >= 0 and (np.abs(U[hit]) < 2.0).all()

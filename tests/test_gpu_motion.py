"""GPU: UH_HYBRID_MOTION. The motion image of the cast and of the rasterised G-buffer on a scene whose panel moves rigidly, deforms and whose
isosurface mesh changes topology, against float64 known answers (tests/motion_reference.py); the mesh states of UhMotionStats; isolation
and the refusals."""
import numpy as np
import pytest

import motion_reference as mr
import rust_renderer_amd as rr
from hybrid_util import add_lights, bits
from motion_util import EXTENT, FLOOR, ISO, PANEL, PANEL_WORLD, SIZES, WALL, MotionRig, mapped, rot
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import quad
from test_gpu_denoise import _state, params
from test_gpu_mesh_deform import device_copy

pytestmark = pytest.mark.gpu

# The device interpolates the triangle's corners in float32 and applies the previous transform in float32; the float64 known answer starts
# from the position texel, which is origin + t * direction (cast) or the interpolated world corners (rasterised) rounded to float32. The
# two differ by float32 rounding of values up to the scene's coordinates (a few units; the matrices' products a few more steps). The
# largest absolute difference over all cases of test_rigid and test_deformed (and the deformation at the end of test_topology), both
# forms, both sizes - 22 figures -, measured on an MI355X, relative to the scene's extent (motion_util.EXTENT = 40): 1.0e-06 absolute,
# a few float32 steps of the panel's coordinates. The bound held is 4 x that (the project's convention).
MOTION_MEASURED = 2.520e-08
MOTION_HELD = 4 * MOTION_MEASURED

FORMS = [pytest.param(False, id="cast"), pytest.param(True, id="raster")]
M_RIGID = rr.transform3x4((1.1, 0.9, 1.2), (0.25, 1.5, 0.3), rot(0.1, -0.25, 0.15))
A1 = np.concatenate([rot(0.05, 0.2, -0.1).astype(np.float64) * np.array([1.05, 0.95, 1.0])[None, :], np.array([[0.1], [-0.05], [0.2]])], axis=1)
A2 = np.concatenate([rot(-0.1, -0.15, 0.05).astype(np.float64) * np.array([0.9, 1.1, 1.0])[None, :], np.array([[-0.15], [0.1], [0.1]])], axis=1)
A3 = np.concatenate([rot(0.0, 0.1, 0.2).astype(np.float64) * np.array([1.0, 1.05, 1.0])[None, :], np.array([[0.05], [0.0], [0.3]])], axis=1)


def compose(*maps):
    """the product of affine maps (row-major 3x4), leftmost applied last, float64"""
    out = np.eye(4)
    for m in maps:
        out = out @ np.concatenate([np.asarray(m, np.float64).reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]]])
    return out[:3]


def assert_verbatim(pos, motion, where, w):
    assert where.any()
    assert np.array_equal(bits(motion[..., :3])[where], bits(pos[..., :3])[where]), "xyz is the position texel's, bit for bit"
    assert (motion[..., 3][where] == w).all()


def assert_states(r, static=0, rigid=0, deformed=0, none=0):
    s = r.gpu.motion_stats()
    assert (s.meshes_static, s.meshes_rigid, s.meshes_deformed, s.meshes_none) == (static, rigid, deformed, none)
    return s


def error(motion, want, where):
    assert where.sum() >= 20, "the panel is on screen"
    assert (motion[..., 3][where] == 1).all()
    e = float(np.abs(motion[..., :3][where].astype(np.float64) - want[where]).max()) / EXTENT
    print(f"motion: largest |device - float64| / extent over {where.sum()} pixels: {e:.3e} (held {MOTION_HELD:.3e})")
    return e


# ---- 1. static ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raster", FORMS)
@pytest.mark.parametrize("size", SIZES)
def test_static(size, raster):
    r = MotionRig(size, raster)
    s0 = r.gpu.motion_stats()  # all zero before the first pass
    assert (s0.pixels_with, s0.pixels_without, s0.meshes_static, s0.motion_ms, s0.snapshot_ms) == (0, 0, 0, 0.0, 0.0)
    for step, shift in enumerate((0.0, 0.3, 0.3)):
        if step == 2:  # the same 12 floats again still count as static
            r.gpu.set_instance_transform(PANEL, PANEL_WORLD)
        pos, mesh, geo, motion = r.gbuffer(r.view(shift))
        assert geo.any() and not geo.all()
        assert {FLOOR, ISO, WALL, PANEL} <= set(np.unique(mesh[geo]).astype(int)), "every mesh is on screen"
        assert_verbatim(pos, motion, geo, 1.0)
        assert not motion[~geo].any(), "not geometry: (0, 0, 0, 0)"
        s = assert_states(r, static=4)
        assert (s.pixels_with, s.pixels_without) == (geo.sum(), 0)
        assert s.motion_ms > 0 and s.snapshot_ms >= 0


# ---- 2. rigid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raster", FORMS)
@pytest.mark.parametrize("size", SIZES)
def test_rigid(size, raster):
    r = MotionRig(size, raster)
    r.gbuffer()
    r.gpu.set_instance_transform(PANEL, M_RIGID)
    pos, mesh, geo, motion = r.gbuffer()
    panel = geo & (mesh == PANEL)
    want = mr.affine(compose(PANEL_WORLD, mr.inverse3x4(M_RIGID)), pos[..., :3])
    assert float(np.abs(want[panel] - pos[..., :3][panel]).max()) > 0.05, "the panel moved"
    assert error(motion, want, panel) <= MOTION_HELD
    assert_verbatim(pos, motion, geo & ~panel, 1.0)
    assert not motion[~geo].any()
    s = assert_states(r, static=3, rigid=1)
    assert (s.pixels_with, s.pixels_without) == (geo.sum(), 0)
    # nothing moved since: the snapshot advanced
    pos, mesh, geo, motion = r.gbuffer()
    assert_verbatim(pos, motion, geo, 1.0)
    assert_states(r, static=4)


# ---- 3. deformed -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raster", FORMS)
@pytest.mark.parametrize("size", SIZES)
def test_deformed(size, raster):
    r = MotionRig(size, raster)
    v0 = r.panel_v
    r.gbuffer()
    worst = 0.0

    def step(vertices, where, want_map, world=None):
        nonlocal worst
        if where == "host":
            r.gpu.update_mesh_vertices(PANEL, vertices)
        else:
            buf = device_copy(vertices)
            r.gpu.update_mesh_vertices(PANEL, device_ptr=buf.ptr, count=len(vertices))
            buf.free()
        if world is not None:
            r.gpu.set_instance_transform(PANEL, world)
        pos, mesh, geo, motion = r.gbuffer()
        panel = geo & (mesh == PANEL)
        assert_states(r, static=3, deformed=1)
        assert_verbatim(pos, motion, geo & ~panel, 1.0)
        if want_map is not None:
            worst = max(worst, error(motion, mr.affine(want_map, pos[..., :3]), panel))
        return pos, panel, motion

    # all vertices under an affine map: the rigid case's known answer, because barycentric interpolation commutes with affine maps (the
    # float32 rounding of the mapped vertices is part of what the margin measures)
    v1 = mapped(v0, A1)
    step(v1, "host", compose(PANEL_WORLD, mr.inverse3x4(A1), mr.inverse3x4(PANEL_WORLD)))
    v2 = mapped(v0, A2)
    step(v2, "device", compose(PANEL_WORLD, A1, mr.inverse3x4(A2), mr.inverse3x4(PANEL_WORLD)))
    # a deformation and a transform change in the same interval
    v3 = mapped(v0, A3)
    step(v3, "host", compose(PANEL_WORLD, A2, mr.inverse3x4(A3), mr.inverse3x4(M_RIGID)), world=M_RIGID)
    # not affine: one interior vertex displaced; the triangle and the barycentrics recovered on the host from the position texel
    v4 = v3.copy()
    v4["pos"][12, :3] += np.float32([0.05, -0.08, 0.3])
    pos, panel, motion = step(v4, "device", None)
    world_now = mr.affine(M_RIGID, v4["pos"][:, :3])[r.panel_i.reshape(-1, 3)]
    tri, b, dist = mr.locate(pos[..., :3][panel], world_now)
    assert dist.max() <= 1e-4, "every panel pixel lies on a triangle of the panel"
    moved = (r.panel_i.reshape(-1, 3)[tri] == 12).any(axis=1)
    assert moved.any() and not moved.all(), "pixels on the triangles around the displaced vertex, and elsewhere"
    xyz, w = mr.motion_texel(mr.DEFORMED, pos[..., :3][panel], v3["pos"][:, :3][r.panel_i.reshape(-1, 3)[tri]], b, M_RIGID)
    want = np.zeros(pos.shape[:2] + (3,))
    want[panel] = xyz
    worst = max(worst, error(motion, want, panel))
    same = mr.affine(compose(M_RIGID, mr.inverse3x4(M_RIGID)), pos[..., :3])
    assert float(np.abs(want[panel] - same[panel]).max()) > 0.05, "the displaced vertex shows"
    print(f"motion: worst of the case {worst:.3e}")
    assert worst <= MOTION_HELD


# ---- 4. topology ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_topology(size):
    r = MotionRig(size)
    pos0, mesh0, geo0, motion0 = r.gbuffer()
    before = r.gpu.read_mesh(ISO)[1].size
    r.gpu.update_isosurface_mesh(ISO, 3.0)
    r.gpu.build_acceleration()
    pos, mesh, geo, motion = r.gbuffer()
    iso = geo & (mesh == ISO)
    assert iso.sum() >= 4
    assert_verbatim(pos, motion, iso, 0.0)
    assert_verbatim(pos, motion, geo & ~iso, 1.0)  # the wall and the panel lie behind it in the vertex table: their vertex_base moved
    s = assert_states(r, static=3, none=1)
    assert (s.pixels_with, s.pixels_without) == ((geo & ~iso).sum(), iso.sum())
    untouched = geo & geo0 & (mesh != ISO) & (mesh0 != ISO)
    assert np.array_equal(bits(motion)[untouched], bits(motion0)[untouched]), "as in the static case"
    pos, mesh, geo, motion = r.gbuffer()
    assert_verbatim(pos, motion, geo, 1.0)
    assert_states(r, static=4)
    # a mesh added before a rebuild behaves the same
    qv, qi = quad((1.8, 0.3, 1.0), (0.9, 0.0, 0.0), (0.0, 0.9, 0.0), nu=2, nv=2)
    new = r.gpu.add_mesh(qv, qi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.9, 0.2, 0.2, 1.0), diffuse_map=r.gpu.default_diffuse_map()))
    r.gpu.build_acceleration()
    pos, mesh, geo, motion = r.gbuffer()
    added = geo & (mesh == new)
    assert added.sum() >= 4
    assert_verbatim(pos, motion, added, 0.0)
    assert_verbatim(pos, motion, geo & ~added, 1.0)
    assert_states(r, static=4, none=1)
    pos, mesh, geo, motion = r.gbuffer()
    assert_verbatim(pos, motion, geo, 1.0)
    assert_states(r, static=5)
    # and the panel can still deform: its rows survived the new layout
    r.gpu.update_mesh_vertices(PANEL, mapped(r.panel_v, A1))
    pos, mesh, geo, motion = r.gbuffer()
    panel = geo & (mesh == PANEL)
    assert_states(r, static=4, deformed=1)
    assert error(motion, mr.affine(compose(PANEL_WORLD, mr.inverse3x4(A1), mr.inverse3x4(PANEL_WORLD)), pos[..., :3]), panel) <= MOTION_HELD
    assert before != r.gpu.read_mesh(ISO)[1].size, "the isosurface's count changed, so the bases behind it moved"


# ---- 5. isolation and refusals ---------------------------------------------------------------------------------------------------
def test_the_bit_changes_nothing_else():
    a, b = MotionRig((67, 45)), MotionRig((67, 45))
    for r, motion in ((a, True), (b, False)):
        add_lights(r.gpu, 4, 7)
        v = r.view()
        v.use_ris_light_sampling = 1
        v.samples_per_frame = 1
        for _ in range(2):
            v.total_samples += 1
            r.gpu.render_frame(v, rr.PASS_ALL)
        r.gpu.render_hybrid(v, r.mask(motion))
        r.gpu.set_instance_transform(PANEL, M_RIGID)
        v.total_samples += 1
        r.gpu.render_frame(v, rr.PASS_ALL)
        r.gpu.render_hybrid(v, r.mask(motion) | rr.HYBRID_FRAME)
    sa, sb = _state(a.gpu), _state(b.gpu)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    ha, hb = a.gpu.hybrid_stats(), b.gpu.hybrid_stats()
    assert tuple(ha.rays) == tuple(hb.rays) and ha.reflection_pixels == hb.reflection_pixels
    assert a.gpu.motion_stats().meshes_rigid == 1 and b.gpu.motion_stats().motion_ms == 0.0


def test_refusals():
    r = MotionRig((40, 24))
    v = r.view()
    r.gpu.render_hybrid(v, rr.HYBRID_MOTION)  # without UH_HYBRID_GBUFFER in the call the bit does nothing
    r.gpu.render_hybrid(v, r.mask(False))
    r.gpu.render_hybrid(v, rr.HYBRID_MOTION | rr.HYBRID_RT_SHADOWS)
    s = r.gpu.motion_stats()
    assert (s.pixels_with, s.pixels_without, s.meshes_static, s.motion_ms) == (0, 0, 0, 0.0)
    with pytest.raises(UtopianError, match="image 15 before the first motion pass"):
        r.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE)
    with pytest.raises(ValueError, match="0..15"):
        r.gpu.read_hybrid(16)
    p = params(iterations=2)
    pm = params(iterations=2, flags=rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE | rr.DENOISE_MOTION)
    v = r.shoot(r.view(), motion=False)
    r.denoise(v, p)
    before = r.images()
    with pytest.raises(UtopianError, match="had no UH_HYBRID_MOTION"):
        r.gpu.denoise(v, pm)
    with pytest.raises(UtopianError, match="image 15 before the first motion pass"):
        r.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE)
    # a motion pass, then a G-buffer pass without the bit: the last pass decides
    r.gpu.render_hybrid(v, r.mask(True))
    assert r.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE).shape == (24, 40, 4)
    r.gpu.render_hybrid(v, r.mask(False))
    with pytest.raises(UtopianError, match="had no UH_HYBRID_MOTION"):
        r.gpu.denoise(v, pm)
    after = r.images()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    # the history survived: the next call of the camera at rest has history 2, with the flag over a motion pass too
    r.denoise(r.shoot(r.view(), motion=True), pm)
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 2).all()
    # the flag without UH_DENOISE_TEMPORAL is accepted and has no effect
    r.denoise(r.shoot(r.view(), motion=True), params(iterations=2, flags=rr.DENOISE_DEMODULATE | rr.DENOISE_MOTION))
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 1).all()

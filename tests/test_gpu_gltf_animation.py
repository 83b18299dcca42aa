"""GPU: a rigged glTF end to end - test_gltf_animation.py's two-joint arm through load_gltf, Renderer.add_model (which hands the skin and
the morph targets to the library) and gltf.Animator.apply at two times of its clip, each followed by a hybrid frame with
view.rebuild_tlas = 1 (G-buffer, ray-traced passes, SSAO, deferred lighting, sky, present). The present image and uh_read_mesh equal,
bit for bit, those of a fresh context whose arm was added with the vertices tests/pose_reference.py computes for that time.
rt_shadows runs ahead of the G-buffer pass, as in the reference's graph, and reads the G-buffer the previous call left: every frame that
is compared is therefore the second call on its geometry, in both contexts."""
import json
import os

import numpy as np
import pytest

import pose_reference as ref
import rust_renderer_amd as rr
import test_gltf_animation as ga
from rust_renderer_amd import gltf
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Scene, quad

pytestmark = pytest.mark.gpu
W, H = 96, 64
LIGHTS = [(4.0, 8.0, 6.0)]
TIMES = (1.5, 2.75)


def make_view(rebuild_tlas):
    cam = Camera((2.0, 4.0, 9.0), (1.0, 3.5, -2.0), 60.0, W / H, 0.01, 1000.0)
    v = Scene("arm", [], LIGHTS, cam, {}).make_view(W, H)
    v.rebuild_tlas = rebuild_tlas
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    return v


def make_ctx(model):
    r = rr.Renderer(W, H)
    r.set_option("device_build", 1)
    ground = r.add_mesh(*quad((-20, 0.0, -20), (0, 0, 40), (40, 0, 0), 4, 4), rr.make_material(base_color=(0.6, 0.6, 0.6, 1.0), diffuse_map=r.default_diffuse_map()))
    ids = r.add_model(model)
    for p in LIGHTS:
        r.add_light(p, (1.0, 0.9, 0.8), 40.0)
    r.build_acceleration()
    return r, ground, ids


IMAGES = dict(position=rr.HYBRID_POSITION, normal=rr.HYBRID_NORMAL, albedo=rr.HYBRID_ALBEDO, pbr=rr.HYBRID_PBR, shadows=rr.HYBRID_SHADOWS,
              reflections=rr.HYBRID_REFLECTIONS, ssao=rr.HYBRID_SSAO_IMAGE, deferred=rr.HYBRID_DEFERRED_OUTPUT, present=rr.HYBRID_PRESENT_OUTPUT)


def frame(r, rebuild_tlas):
    """a hybrid frame with view.rebuild_tlas as given, then the same frame again, whose rt_shadows pass sees this geometry's G-buffer:
    every image of the second, in pass order (present last)"""
    r.render_hybrid(make_view(rebuild_tlas), rr.HYBRID_FRAME)
    r.render_hybrid(make_view(0), rr.HYBRID_FRAME)
    return {name: r.read_hybrid(k) for name, k in IMAGES.items()}


def assert_same_frame(a, b, what):
    for name in IMAGES:  # the first pass that differs names itself
        x, y = (np.ascontiguousarray(i).view(np.uint8) for i in (a[name], b[name]))
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {name} differs in {np.count_nonzero(x != y)} of {x.size} bytes"


def test_the_animated_arm_renders_as_a_fresh_context_fed_the_reference_vertices(tmp_path):
    path = os.path.join(str(tmp_path), "arm.gltf")
    with open(path, "w") as f:
        json.dump(ga.arm_gltf(), f)
    model = gltf.load_gltf(path)
    arm = model.meshes[0]
    a, _, ids = make_ctx(model)
    assert a.pose_stats().poses == 0
    rest = frame(a, 0)["present"]
    anim = gltf.Animator(model)
    shown = []
    for t in TIMES:
        anim.apply(a, ids, 0, t)
        shown_a = frame(a, 1)
        (jm, mw), = anim.pose(0, t).values()
        want = ref.pose(arm.vertices, arm.joints, arm.weights, jm, arm.morph_positions, arm.morph_normals, mw)
        got, idx = a.read_mesh(ids[0])
        assert got.tobytes() == want.tobytes() and np.array_equal(idx, arm.indices), f"the arm at t = {t}"
        fresh = gltf.load_gltf(path)
        fresh.meshes[0].vertices = want
        fresh.meshes[0].skin = fresh.meshes[0].morph_positions = None  # an unrigged mesh: add_model sets nothing on it
        b, _, fresh_ids = make_ctx(fresh)
        assert_same_frame(shown_a, frame(b, 0), f"t = {t}")
        assert b.read_mesh(fresh_ids[0])[0].tobytes() == got.tobytes() and b.pose_stats().poses == 0
        shown.append(shown_a["present"])
    assert not np.array_equal(shown[0], rest) and not np.array_equal(shown[0], shown[1]), "the arm moved on screen"
    s = a.pose_stats()
    assert (s.poses, s.vertices, s.joints, s.active_targets) == (2, len(arm.vertices), 2, 2)

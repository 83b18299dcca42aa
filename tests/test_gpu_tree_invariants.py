"""GPU: every tree whose nodes the device wrote - the PLOC and radix builders of csrc/lbvh.hip, every refit (csrc/refit.hip, which
all device builds end in), the device route of update_isosurface_mesh - and the host builder's beside them, read back by
check_acceleration and held to the builders' invariants (csrc/bvh_invariants.h): boxes contain their subtrees, every packet and
node is reachable exactly once, n_tri / n_child are right, no child lies in an earlier refit level, the packets are the bake of the
corners, the keys are the scene's. The same statement is calibrated on the host builder's trees and shown to find planted faults by
tests/cpp/bvh_check.cpp (test_sanitizers.py). Ray tests sample a tree; this walks it.

Device-built trees differ from run to run in slot order (the collapse's atomics), so nothing here compares bytes. Every case
prints a line `TREE scene | builder | nodes | levels | SAH figure` (profiles/tree_invariants.txt); no bound is asserted on the
figure."""
import functools

import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Mesh, Model, Scene, _pack_vertices
from test_gpu_isosurface_update import ISO, SPHERE, T_HALF_PI, make_ctx, oracle
from test_gpu_parity import _chain_scene, _rot, _single_triangle_scene, _soup_scene
from util import far_scene, run_frames, torture_scene

pytestmark = pytest.mark.gpu

BUILDERS = [0, 1, (1, 0), (1, 24), 2]  # option device_build, or (device_build, ploc_sah_top): (1, 0) = PLOC rounds to the root
MAX_TREE_LEVELS = (16 + 96) // 3       # bvh.h kMaxTreeLevels
MISS = 0xFFFFFFFF


def _name(builder):
    return {0: "host", 1: "ploc+sah_top", (1, 0): "ploc to the root", (1, 24): "ploc, top 24", 2: "radix"}[builder]


def _renderer(builder, W=16, H=16):
    r = rr.Renderer(W, H)
    kind, top = builder if isinstance(builder, tuple) else (builder, None)
    r.set_option("device_build", kind)
    if top is not None:
        r.set_option("ploc_sah_top", top)
    return r


def _sound(r, scene_name, builder, triangles=None, step=""):
    """all violation counts are zero; prints the table's line"""
    rep = r.check_acceleration()
    print(f"TREE {scene_name}{' / ' + step if step else ''} | {_name(builder)} | {rep['nodes']} | {rep['levels']} | {rep['sah']:.3f}")
    assert rep["violations"] == dict.fromkeys(rep["violations"], 0), rep["first"]
    assert rep["first"] == "" and rep["geometry_checked"]
    assert 1 <= rep["levels"] <= MAX_TREE_LEVELS and rep["nodes"] >= 1
    if triangles is not None:
        assert rep["triangles"] == triangles
    return rep


def _soup_mesh(pos):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    return Mesh(_pack_vertices(pos, np.tile(np.float32([0, 0, 1]), (len(pos), 1)), np.zeros((len(pos), 2), np.float32)), np.arange(len(pos), dtype=np.uint32))


def _soup(name, pos):
    return Scene(name, [(Model([_soup_mesh(pos)], []), None)], [], Camera((0, 0, 6), (0, 0, 0), 60.0, 1.0, 0.01, 100.0))


def _overflowing_scene():
    """the scene of test_device_build_falls_back_to_the_host_builder_on_overflowing_geometry: coordinates around 3e19"""
    rng = np.random.default_rng(11)
    c = rng.uniform(-1, 1, (400, 1, 3)) * 3e19
    return _soup("huge", c + rng.uniform(-1, 1, (400, 3, 3)) * 2e18)


# bvh_check.cpp's degenerate soups as scenes
def _identical():
    return _soup("1000 identical triangles", np.tile(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), (1000, 1, 1)))  # every Morton code equal


def _points():
    return _soup("5000 point triangles", np.repeat(np.random.default_rng(7).uniform(0, 1, (5000, 1, 3)), 3, axis=1))


def _sheet():
    rng = np.random.default_rng(8)
    x, z = rng.uniform(0, 10, 20000), rng.uniform(0, 10, 20000)
    zero = np.zeros_like(x)
    return _soup("20000-triangle coplanar sheet", np.stack([np.stack([x, zero, z], -1), np.stack([x + 0.1, zero, z], -1), np.stack([x, zero, z + 0.1], -1)], 1))


def _million():
    return _soup("3000 triangles at +-1e6", np.random.default_rng(9).uniform(-1e6, 1e6, (3000, 3, 3)))


@functools.lru_cache(maxsize=None)
def _scene(which):
    return {
        "cornell": lambda: rr.scenes.cornell_scene(subdivisions=2, tex_size=16),
        "atrium": lambda: rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=64, sphere_subdivisions=2),
        "torture": torture_scene,
        "soup11": lambda: _soup_scene(11),
        "one": _single_triangle_scene,
        "empty": lambda: Scene("empty", [(Model([], []), None)], [], Camera((0, 0, 4), (0, 0, 0), 60.0, 1.0, 0.01, 100.0)),
        "far_grid": lambda: far_scene("grid"),
        "far_grid_at_1000": lambda: far_scene("grid_at_1000"),
        "identical": _identical,
        "points": _points,
        "sheet": _sheet,
        "million": _million,
    }[which]()


SCENES = ["cornell", "atrium", "torture", "soup11", "one", "empty", "far_grid", "far_grid_at_1000", "identical", "points", "sheet", "million"]


# ---- 1. the builders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS, ids=str)
@pytest.mark.parametrize("which", SCENES)
def test_every_builder_leaves_a_sound_tree(which, builder):
    scene = _scene(which)
    r = scene.upload(_renderer(builder))
    _sound(r, which, builder, scene.num_triangles)


# ---- 2. the two fallbacks: what was installed in the end ---------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS, ids=str)
@pytest.mark.parametrize("which", ["chain", "overflow"])
def test_the_tree_a_fallback_installs_is_sound(which, builder):
    """a scene whose SAH and Morton trees are deeper than the traversal stack (the host builder rebuilds balanced, a device build
    hands over to it), and one whose area products overflow (a PLOC round merges nothing: host builder)"""
    scene = _chain_scene() if which == "chain" else _overflowing_scene()
    r = scene.upload(_renderer(builder))
    _sound(r, which, builder, scene.num_triangles)


# ---- 3. triangle counts at the edges of the collapse and of device_scan.h's 2,048-value chunk -------------------------------
EDGE_COUNTS = [2, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4097]
N_AIMED = 2000


@functools.lru_cache(maxsize=None)
def _edge_case(n):
    """the soup of n triangles, 2,000 rays aimed at points of its triangles (a third inside one, a third on an edge, a third at a
    vertex, so that a box a step too small shows) and what the oracle's brute force answers: once per n, never written to"""
    rng = np.random.default_rng(5000 + n)
    pos = (rng.uniform(-2, 2, (n, 1, 3)) + rng.normal(scale=0.3, size=(n, 3, 3))).astype(np.float32)
    scene = _soup(f"soup of {n}", pos)
    w = rng.dirichlet((1.0, 1.0, 1.0), N_AIMED)
    k = np.arange(N_AIMED) % 3
    w[k == 1, 2] = 0.0
    w[k == 1] /= w[k == 1].sum(axis=1, keepdims=True)
    w[k == 2] = np.eye(3)[rng.integers(0, 3, int((k == 2).sum()))]
    target = np.einsum("rv,rva->ra", w, pos[rng.integers(0, n, N_AIMED)].astype(np.float64)).astype(np.float32)
    origin = (rng.normal(size=(N_AIMED, 3)) * 6.0).astype(np.float32)
    rays = np.empty((N_AIMED, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 0.001, target - origin, 10000.0
    cpu = scene.upload(oa.OracleRenderer(8, 8, brute_force=True))
    tuv, mesh, prim = cpu.trace_closest(rays)
    occluded = cpu.trace_any(rays)
    for a in (rays, tuv, mesh, prim, occluded):
        a.setflags(write=False)
    return scene, rays, tuv, mesh, prim, occluded


@pytest.mark.parametrize("builder", [(1, 0), 2], ids=str)
@pytest.mark.parametrize("n", EDGE_COUNTS)
def test_edge_triangle_counts_build_sound_trees_that_keep_every_hit(n, builder):
    scene, rays, tuv, mesh, prim, occluded = _edge_case(n)
    r = scene.upload(_renderer(builder))
    _sound(r, scene.name, builder, n)
    assert (mesh != MISS).mean() > 0.5, "the rays must hit what they are aimed at"
    tg, mg, pg = r.trace_closest(rays)
    assert np.array_equal(mg, mesh) and np.array_equal(pg, prim)
    assert np.array_equal(tg.view(np.uint32), tuv.view(np.uint32)), "t / u / v must equal brute force bit for bit"
    assert np.array_equal(r.trace_any(rays), occluded)


# ---- 4. refit ------------------------------------------------------------------------------------------------------------------
def _atrium_moves(n_mesh):
    """the three moves of test_refit_equals_rebuild_bit_for_bit"""
    return [(n_mesh - 1, rr.transform3x4((0.8, 1.1, 0.9), (1.5, 0.7, -0.4), _rot(0.3, 1.0, -0.2))),
            (n_mesh - 2, rr.transform3x4((1.0, 1.0, 1.0), (-2.0, 1.2, 0.6))),
            (3, rr.transform3x4((1.02, 0.97, 1.0), (0.05, 0.0, -0.03), _rot(0.0, 0.02, 0.0)))]


@pytest.mark.parametrize("how", ["refit", "flag"])
@pytest.mark.parametrize("builder", BUILDERS, ids=str)
def test_refitted_atrium_is_sound(builder, how):
    scene = _scene("atrium")
    W, H = 48, 32
    r = scene.upload(_renderer(builder, W, H))
    run_frames(r, scene, W, H, 1, rr.PASS_REFERENCE_PT)  # frames in flight on the old tree
    for mesh, w in _atrium_moves(scene.num_meshes):
        r.set_instance_transform(mesh, w)
    if how == "refit":
        r.rebuild_tlas()
    else:
        run_frames(r, scene, W, H, 1, rr.PASS_REFERENCE_PT, rebuild_tlas=1)  # as the application asks for it: the view flag
    _sound(r, "atrium", builder, scene.num_triangles, step="moved, " + how)


@pytest.mark.parametrize("builder", BUILDERS, ids=str)
def test_refit_of_mirrored_and_scaled_instances_and_onto_itself(builder):
    scene = _scene("torture")
    r = scene.upload(_renderer(builder))
    before = _sound(r, "torture", builder, scene.num_triangles)
    r.rebuild_tlas()  # nothing moved: the same boxes again
    same = _sound(r, "torture", builder, scene.num_triangles, step="refit onto itself")
    assert (same["nodes"], same["levels"]) == (before["nodes"], before["levels"]) and same["sah"] == before["sah"]
    r.set_instance_transform(7, rr.transform3x4((-0.7, 1.5, -1.0), (0.4, -0.1, 0.3), _rot(0.4, -0.2, 1.1)))   # the mirrored instance
    r.set_instance_transform(8, rr.transform3x4((2e-3, 5e-4, 1.0), (-0.6, 0.2, 1.25), _rot(0.0, 0.0, 0.5)))  # the 1e-3-scaled one
    r.rebuild_tlas()
    _sound(r, "torture", builder, scene.num_triangles, step="instances 7, 8 moved")
    r.set_instance_transform(7, rr.transform3x4((0.5, -2.0, 1.0), (0.1, 0.2, -1.0)))
    r.rebuild_tlas()
    _sound(r, "torture", builder, scene.num_triangles, step="instance 7 moved back")


@pytest.mark.parametrize("builder", BUILDERS, ids=str)
@pytest.mark.parametrize("kind", ["grid", "grid_at_1000"])
def test_refit_after_the_wall_is_put_back(kind, builder):
    scene = far_scene(kind, wall_moved=True)
    r = scene.upload(_renderer(builder))
    r.set_instance_transform(1, rr.identity3x4())
    r.rebuild_tlas()
    _sound(r, "far_" + kind, builder, scene.num_triangles, step="wall put back")


# ---- 5. isosurface updates -----------------------------------------------------------------------------------------------------
ISO_STATICS = 128 + 320 + 12  # triangles of the ground, the sphere and the box (test_gpu_isosurface_update.make_ctx)


@pytest.mark.parametrize("device_build", [0, 1])
@pytest.mark.parametrize("window", ["grows", "empties"])
def test_updated_isosurface_meshes_leave_sound_trees(window, device_build):
    """add_isosurface_mesh(32, ...), then update_isosurface_mesh to a time that grows the mesh, or to one that empties it and to
    one that brings it back; a check after each step and after a refit of the updated mesh"""
    res = 32
    lo, hi, times = {"grows": (0.0, 32.0, (0.0, 3.0)), "empties": (21.5, 24.5, (T_HALF_PI, 0.0, T_HALF_PI))}[window]
    count = [oracle(res, t, lo, hi, positions=False)["triangles"] for t in times]
    assert count[1] > count[0] if window == "grows" else (count[1] == 0 and count[0] > 0)
    r = make_ctx(res, times[0], device_build, lo, hi)
    _sound(r, f"isosurface {window}", device_build, ISO_STATICS + count[0], step=f"t = {times[0]:g}")
    for t, n in zip(times[1:], count[1:]):
        assert r.update_isosurface_mesh(ISO, t) == n
        with pytest.raises(rr.UtopianError):
            r.check_acceleration()  # the mesh has changed: no tree for the scene as it is
        r.build_acceleration()
        _sound(r, f"isosurface {window}", device_build, ISO_STATICS + n, step=f"updated to t = {t:g}")
    r.set_instance_transform(ISO, rr.transform3x4((1.1, 0.9, 1.0), (0.5, -0.25, 0.75), _rot(0.1, 0.3, -0.2)))
    r.set_instance_transform(SPHERE, rr.transform3x4((3, 3, 3), (5.0, 9.5, 25.0)))
    r.rebuild_tlas()
    _sound(r, f"isosurface {window}", device_build, ISO_STATICS + count[-1], step="updated mesh moved, refit")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_check_acceleration_needs_a_built_tree():
    r = rr.Renderer(16, 16)
    with pytest.raises(rr.UtopianError, match="INVALID_ARGUMENT"):
        r.check_acceleration()
    scene = _scene("cornell")
    for model, transform in scene.models:
        r.add_model(model, transform)
    with pytest.raises(rr.UtopianError, match="INVALID_ARGUMENT"):
        r.check_acceleration()  # meshes, but no build yet
    r.initialize_raytracing()
    _sound(r, "cornell", 0, scene.num_triangles, step="after the refusals")

"""GPU: posed meshes - uh_set_mesh_skin / uh_set_mesh_morph_targets / uh_pose_mesh / uh_get_pose_stats. k_pose is held, bit for bit, to
tests/pose_reference.py (the numpy float32 restatement of DESIGN.md section 2 "Posed meshes") through uh_read_mesh, over every vertex
and joint count at which the kernel takes another path; the state a pose leaves is held to that of a fresh context made with
uh_add_mesh from the reference's vertices (traces, path-traced frames, both G-buffers, motion vectors), on test_gpu_mesh_deform.py's
scene with the sheet replaced by a tube that three joints bend. Pose 1 of the tube lies wholly outside the box of pose 0: boxes left
stale would lose hits. Finite inputs only: nothing here provokes a device fault."""
import functools

import numpy as np
import pytest

import pose_reference as ref
import rust_renderer_amd as rr
import test_gpu_mesh_deform as md
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import box, cylinder, icosphere, quad
from rust_renderer_amd.types import VERTEX_DTYPE

pytestmark = pytest.mark.gpu
GROUND, SPHERE, TUBE, BOX = range(4)  # the posed mesh is neither first nor last
TUBE_JOINTS, TUBE_TARGETS = 3, 3
VERTEX_COUNTS = (1, 63, 64, 65, 255, 256, 257)
JOINT_COUNTS = (1, 3, 64, 65, 256, 257, 1024, 1025)
STAGED_LIMIT = 0  # k_pose reads the matrices through L2 at every joint count: there is no second route, and no limit to straddle


# ---- the tube ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tube():
    """a tube of radius 1.5 along y in [-6, 6], 17 x 25 vertices with unit tangents (w = -1), three joints along it with smooth weights
    in the first three slots (the fourth weighs nothing), three morph targets with normal deltas"""
    v, idx = cylinder((0.0, -6.0, 0.0), 1.5, 12.0, 16, 24)
    v = v.copy()
    y = v["pos"][:, 1].astype(np.float64)
    v["tangent"][:, :3] = (0.0, 1.0, 0.0)
    v["tangent"][:, 3] = -1.0
    centres = np.array([-4.0, 0.0, 4.0])
    w = np.exp(-((y[:, None] - centres[None, :]) / 3.0) ** 2)
    weights = np.zeros((len(v), 4), dtype=np.float32)
    weights[:, :3] = w / w.sum(axis=1, keepdims=True)
    joints = np.tile(np.array([0, 1, 2, 0], dtype=np.uint16), (len(v), 1))
    radial = v["pos"][:, :3].astype(np.float64) * (1.0, 0.0, 1.0) / 1.5
    dp = np.stack([radial * np.sin(0.5 * y)[:, None] * 0.4, radial * np.cos(0.9 * y)[:, None] * 0.3, radial * 0.25]).astype(np.float32)
    dn = np.stack([np.stack([0 * y, 0.3 * np.cos(0.5 * y), 0 * y], axis=1), np.stack([0 * y, -0.2 * np.sin(0.9 * y), 0 * y], axis=1),
                   np.zeros((len(v), 3))]).astype(np.float32)
    for a in (v, idx, joints, weights, dp, dn):
        a.setflags(write=False)
    return v, idx, joints, weights, dp, dn


def _rot_x(angle, pivot_y):
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[1:3, 1:3] = [[c, -s], [s, c]]
    m[:3, 3] = np.array([0.0, pivot_y, 0.0]) - m[:3, :3] @ np.array([0.0, pivot_y, 0.0])
    return m


@functools.lru_cache(maxsize=None)
def tube_pose(k):
    """(joint matrices (3, 12), morph weights (3,)) of pose k: a chain of three joints that bends about x (the tube stays in its own x
    range), the whole shifted to x = -5 (even k) or x = +5 (odd k); the second target's weight is exactly zero"""
    g = np.eye(4)
    g[0, 3] = 5.0 if k % 2 else -5.0
    mats = []
    for pivot, angle in zip((-6.0, -2.0, 2.0), (0.15 + 0.1 * k, -0.35 - 0.05 * k, 0.5 - 0.2 * k)):
        g = g @ _rot_x(angle, pivot)
        mats.append(g[:3, :].reshape(12))
    jm, mw = np.array(mats, dtype=np.float32), np.array([0.7 - 0.2 * k, 0.0, 0.4 + 0.1 * k], dtype=np.float32)
    jm.setflags(write=False), mw.setflags(write=False)
    return jm, mw


@functools.lru_cache(maxsize=None)
def tube_posed(k):
    v, _, joints, weights, dp, dn = tube()
    out = ref.pose(v, joints, weights, tube_pose(k)[0], dp, dn, tube_pose(k)[1])
    out.setflags(write=False)
    return out


def fill_scene(r, tube_vertices):
    def mat(*rgb):
        return rr.make_material(base_color=rgb + (1.0,), diffuse_map=r.default_diffuse_map())

    assert r.add_mesh(*quad((-64, 4.99, -64), (0, 0, 160), (160, 0, 0), 8, 8), mat(0.6, 0.6, 0.6)) == GROUND
    assert r.add_mesh(*icosphere(2), mat(0.8, 0.3, 0.2), md.SPHERE_WORLD) == SPHERE
    assert r.add_mesh(tube_vertices, tube()[1], mat(0.8, 0.8, 0.8), md.DEFORM_WORLD) == TUBE
    assert r.add_mesh(*box((27.0, 7.5, 8.0), (2.0, 2.5, 2.0)), mat(0.2, 0.4, 0.8)) == BOX
    for p in md.LIGHTS:
        r.add_light(p, (1.0, 0.9, 0.8), 40.0)
    return r


def make_ctx(tube_vertices, device_build, rigged=False):
    r = rr.Renderer(md.W, md.H)
    r.set_option("sun_grid_force", 1)
    r.set_option("device_build", device_build)
    fill_scene(r, tube_vertices)
    r.build_acceleration()
    if rigged:
        rig(r)
    return r


def rig(r):
    _, _, joints, weights, dp, dn = tube()
    r.set_mesh_skin(TUBE, joints, weights, TUBE_JOINTS)
    r.set_mesh_morph_targets(TUBE, dp, dn)


def pose_tube(r, k):
    r.pose_mesh(TUBE, *tube_pose(k))


def gbuffers(r):
    """the cast and the rasterised G-buffer"""
    v = md.make_view()
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    r.render_hybrid(v, rr.HYBRID_GBUFFER)
    out = {"cast_" + name: r.read_hybrid(k) for name, k in (("position", rr.HYBRID_POSITION), ("normal", rr.HYBRID_NORMAL), ("albedo", rr.HYBRID_ALBEDO))}
    out.update(md.one_raster(r))
    return out


def assert_bits(got, want, what):
    assert got.dtype == want.dtype == VERTEX_DTYPE and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        for field in VERTEX_DTYPE.names:
            x, y = got[field].view(np.uint32), want[field].view(np.uint32)
            bad = np.argwhere(x != y)
            assert not len(bad), f"{what}: {field} differs in {len(bad)} words, first at {tuple(bad[0])}: {got[field][tuple(bad[0])]!r} != {want[field][tuple(bad[0])]!r}"


def test_the_poses_are_what_the_tests_below_rely_on():
    p0, p1 = tube_posed(0), tube_posed(1)
    assert p0["pos"][:, 0].max() < -3.0 and p1["pos"][:, 0].min() > 3.0, "pose 1 lies wholly outside the (padded) box of pose 0"
    assert np.isfinite(p0["pos"]).all() and np.isfinite(p1["pos"]).all()
    assert np.allclose(np.linalg.norm(p1["normal"][:, :3], axis=1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(p1["tangent"][:, :3], axis=1), 1.0, atol=1e-6) and (p1["tangent"][:, 3] == -1.0).all()
    assert tube_pose(0)[1][1] == 0.0 and len(tube()[0]) == 17 * 25


# ---- 1. uh_read_mesh after a pose equals the reference, bit for bit ------------------------------------------------------------------
def random_bind(rng, n):
    v = np.zeros(n, dtype=VERTEX_DTYPE)
    for field in VERTEX_DTYPE.names:
        v[field] = rng.uniform(-2.0, 2.0, v[field].shape).astype(np.float32)
    v["tangent"][::5, :3] = 0.0  # what the loader writes for an asset without tangents: stays zero
    v["normal"][::7, :3] = 0.0
    v["_pad"] = rng.integers(0, 2**32, v["_pad"].shape, dtype=np.uint32).view(np.float32)  # any bits, NaN patterns among them
    v["color"][::3, 1] = np.float32(np.nan)
    return v


def random_skin(rng, n, nj):
    joints = rng.integers(0, nj, (n, 4)).astype(np.uint16)
    joints[::2, 3] = nj - 1  # the last joint is read
    weights = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)  # they do not sum to one
    weights[rng.uniform(size=(n, 4)) < 0.3] = 0.0
    weights[:, 0] = np.maximum(weights[:, 0], np.float32(0.1))
    mats = np.tile(np.eye(3, 4), (nj, 1, 1)) + rng.uniform(-0.3, 0.3, (nj, 3, 4))
    if nj >= 3:
        mats[1, :, :3] = np.diag([-1.0, 1.0, 1.0])  # mirrored
        mats[2, :, :3] = np.eye(3) * 1e-3           # scaled to a thousandth
    mats[nj - 1, :, 3] += 3.0
    return joints, weights, mats.astype(np.float32).reshape(nj, 12)


def random_morph(rng, n, T, normals):
    dp = rng.uniform(-0.5, 0.5, (T, n, 3)).astype(np.float32)
    dn = rng.uniform(-0.5, 0.5, (T, n, 3)).astype(np.float32) if normals else None
    mw = rng.uniform(-1.0, 1.0, T).astype(np.float32)
    mw[1::3] = 0.0  # some weights exactly zero (T = 7: targets 1 and 4)
    return dp, dn, mw


def check_pose(r, mesh, rng, nj, T, normals, what):
    """sets a random skin of nj joints (0: none) and T random targets (0: none) on the mesh's current vertices, poses, compares"""
    bind = r.read_mesh(mesh)[0]
    n = len(bind)
    kw = {}
    if nj:
        joints, weights, mats = random_skin(rng, n, nj)
        r.set_mesh_skin(mesh, joints, weights, nj)
        kw.update(joints=joints, weights=weights, joint_matrices=mats)
    if T:
        dp, dn, mw = random_morph(rng, n, T, normals)
        r.set_mesh_morph_targets(mesh, dp, dn)
        kw.update(position_deltas=dp, normal_deltas=dn, morph_weights=mw)
    r.pose_mesh(mesh, kw.get("joint_matrices"), kw.get("morph_weights"))
    want = ref.pose(bind, **kw)
    assert np.isfinite(want["pos"][:, :3]).all()
    assert_bits(r.read_mesh(mesh)[0], want, what)
    s = r.pose_stats()
    assert (s.vertices, s.joints, s.active_targets) == (n, nj, 0 if not T else int(np.count_nonzero(kw["morph_weights"])))
    return s


def shape_meshes(r, rng):
    """a mesh per vertex count, the tube's among them, each with one degenerate triangle: a pose needs no tree"""
    mat = rr.make_material(diffuse_map=r.default_diffuse_map())
    return [(r.add_mesh(random_bind(rng, n), np.zeros(3, np.uint32), mat), n) for n in VERTEX_COUNTS + (len(tube()[0]),)]


@pytest.mark.parametrize("nj", JOINT_COUNTS)
def test_read_mesh_after_a_skinned_pose_equals_the_reference(nj):
    rng = np.random.default_rng(100 + nj)
    r = rr.Renderer(16, 16)
    for T, normals in ((0, False), (7, True)):
        for mesh, n in shape_meshes(r, rng):
            s = check_pose(r, mesh, rng, nj, T, normals, f"{n} vertices, {nj} joints, {T} targets")
            assert s.staged_joint_limit == STAGED_LIMIT, "a limit other than zero, and that limit + 1, belong in JOINT_COUNTS"


@pytest.mark.parametrize("skin,T,normals", [(skin, T, normals) for skin in (False, True) for T in (0, 1, 7) for normals in (False, True)
                                            if (skin or T) and (T or not normals)])
def test_read_mesh_after_a_pose_equals_the_reference_for_every_combination_of_parts(skin, T, normals):
    rng = np.random.default_rng(7 + 2 * T + normals)
    r = rr.Renderer(16, 16)
    for mesh, n in shape_meshes(r, rng):
        check_pose(r, mesh, rng, 3 if skin else 0, T, normals, f"{n} vertices, skin {skin}, {T} targets, normals {normals}")


def test_a_second_pose_writes_the_buffer_the_first_one_retired():
    rng = np.random.default_rng(11)
    n, nj = 300, 64
    bind = random_bind(rng, n)
    joints, weights, mats = random_skin(rng, n, nj)
    dp, dn, mw = random_morph(rng, n, 4, True)
    r = rr.Renderer(16, 16)
    mesh = r.add_mesh(bind, np.zeros(3, np.uint32), rr.make_material(diffuse_map=r.default_diffuse_map()))
    r.set_mesh_skin(mesh, joints, weights, nj)
    r.set_mesh_morph_targets(mesh, dp, dn)
    for k in range(4):  # the two vertex buffers change places with every pose
        jm = mats if k % 2 == 0 else mats[::-1].copy()
        r.pose_mesh(mesh, jm, mw)
        assert_bits(r.read_mesh(mesh)[0], ref.pose(bind, joints, weights, jm, dp, dn, mw), f"pose {k}")


# ---- 2. equivalence with a fresh context ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["refit", "build"])
@pytest.mark.parametrize("device_build", [0, 1, 2])
def test_a_pose_equals_a_fresh_context(device_build, how):
    a = make_ctx(tube()[0], device_build, rigged=True)
    pose_tube(a, 0)
    md.way_out(a, how)
    _, s = md.path_traced(a)  # both grids and the raster tables settle on pose 0
    md.assert_grids(s)
    before, old = md.traced(a), gbuffers(a)
    moved = a.mesh_update_stats().host_geometry_bytes
    pose_tube(a, 1)
    md.way_out(a, how)
    if device_build:
        assert a.mesh_update_stats().host_geometry_bytes == moved, "a pose and its way out moved geometry through the host"
    md.assert_sound(a)
    b = make_ctx(tube_posed(1), device_build)
    ta, tb = md.traced(a), md.traced(b)
    md.assert_same(ta, tb, "traces")
    assert np.count_nonzero(ta["mesh"] == TUBE) > 50 and not np.array_equal(ta["tuv"], before["tuv"])
    (pa, sa), (pb, sb) = md.path_traced(a), md.path_traced(b)
    md.assert_same(pa, pb, "frames")
    md.assert_grids(sa), md.assert_grids(sb)
    ga = gbuffers(a)
    md.assert_same(ga, gbuffers(b), "G-buffers")
    for k in ("cast_position", "gbuffer_depth"):
        assert not np.array_equal(md.bits(ga[k]), md.bits(old[k])), f"{k}: the pose changed nothing"
    assert_bits(a.read_mesh(TUBE)[0], tube_posed(1), "the tube")
    assert np.array_equal(a.read_mesh(TUBE)[1], tube()[1])


# ---- 3. motion vectors ------------------------------------------------------------------------------------------------------------------
def test_motion_vectors_follow_a_posed_mesh_as_they_follow_an_updated_one():
    def motion_frame(r):
        v = md.make_view(rebuild_tlas=1)
        v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
        r.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_MOTION)
        return r.read_hybrid(rr.HYBRID_MOTION_IMAGE), r.read_hybrid(rr.HYBRID_POSITION)

    a, b = make_ctx(tube()[0], 1, rigged=True), make_ctx(tube()[0], 1)
    images = []
    for r, posed in ((a, True), (b, False)):
        motion_frame(r)
        for k in (0, 1):
            pose_tube(r, k) if posed else r.update_mesh_vertices(TUBE, tube_posed(k))
            motion, position = motion_frame(r)
            s = r.motion_stats()
            assert (s.meshes_static, s.meshes_deformed) == (3, 1)
        images.append((motion, position))
    assert np.array_equal(md.bits(images[0][0]), md.bits(images[1][0])) and np.array_equal(md.bits(images[0][1]), md.bits(images[1][1]))
    moved = np.abs(images[0][0][..., :3] - images[0][1][..., :3]).max(axis=-1) > 1.0
    assert moved.sum() > 50, "the tube went from x = -5 to x = +5: its pixels' previous positions lie far from their present ones"


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def refused(call, match):
    with pytest.raises(UtopianError, match=match) as e:
        call()
    assert "INVALID_ARGUMENT" in str(e.value), e.value


def test_an_overflowing_pose_is_refused_and_changes_nothing():
    a = make_ctx(tube()[0], 1, rigged=True)
    pose_tube(a, 0)
    a.rebuild_tlas()
    before, frame = md.traced(a), gbuffers(a)
    stats = a.pose_stats()
    updates = a.mesh_update_stats().updates
    jm = tube_pose(1)[0].copy()
    jm[:, 3] = np.float32(3e38)  # finite, but two of them blended with weights near a half each and added to x overflow
    jm[:, 0] = np.float32(3e38)
    refused(lambda: a.pose_mesh(TUBE, jm, tube_pose(1)[1]), "not finite")
    # still built: no refit, no build, and the same answers
    md.assert_same(md.traced(a), before, "traces after the refusal")
    md.assert_same(gbuffers(a), frame, "G-buffers after the refusal")
    assert_bits(a.read_mesh(TUBE)[0], tube_posed(0), "the tube after the refusal")
    after = a.pose_stats()
    assert (after.poses, after.vertices, after.joints) == (stats.poses, stats.vertices, stats.joints) and a.mesh_update_stats().updates == updates
    pose_tube(a, 1)  # and the mesh can still be posed
    assert_bits(a.read_mesh(TUBE)[0], tube_posed(1), "the tube after a later pose")


def test_argument_errors_leave_the_scene_as_it_was():
    a = make_ctx(tube()[0], 1, rigged=True)
    iso, _ = a.add_isosurface_mesh(8, 21.5, 24.5, md.T_HALF_PI)
    a.build_acceleration()
    pose_tube(a, 0)
    a.rebuild_tlas()
    before = md.traced(a)
    v, _, joints, weights, dp, dn = tube()
    n = len(v)
    jm, mw = tube_pose(1)

    def poisoned(x, value, at):
        x = x.copy()
        x[at] = value
        return x

    lib, ctx = a._lib, a._ctx
    skin, morph, pose = a._uh("set_mesh_skin"), a._uh("set_mesh_morph_targets"), a._uh("pose_mesh")
    jp, wp, dpp, jmp, mwp = joints.ctypes.data, weights.ctypes.data, dp.ctypes.data, jm.ctypes.data, mw.ctypes.data
    raw = lambda fn, *args: a._check(fn(ctx, *args))
    cases = {
        "skin: bad index": (lambda: a.set_mesh_skin(99, joints, weights, 3), "bad mesh index"),
        "skin: isosurface mesh": (lambda: a.set_mesh_skin(iso, np.zeros((3, 4), np.uint16), np.ones((3, 4), np.float32), 1), "isosurface"),
        "skin: wrong count": (lambda: a.set_mesh_skin(TUBE, joints[:-1], weights[:-1], 3), "vertex count"),
        "skin: no joints": (lambda: a.set_mesh_skin(TUBE, joints, weights, 0), "num_joints"),
        "skin: null joints": (lambda: raw(skin, TUBE, None, wp, n, 3), "null"),
        "skin: null weights": (lambda: raw(skin, TUBE, jp, None, n, 3), "null"),
        "skin: joint out of range": (lambda: a.set_mesh_skin(TUBE, poisoned(joints, 3, (n - 1, 3)), weights, 3), "out of range"),
        "skin: negative weight": (lambda: a.set_mesh_skin(TUBE, joints, poisoned(weights, -0.25, (5, 1)), 3), "negative or not finite"),
        "skin: NaN weight": (lambda: a.set_mesh_skin(TUBE, joints, poisoned(weights, np.nan, (5, 1)), 3), "negative or not finite"),
        "skin: inf weight": (lambda: a.set_mesh_skin(TUBE, joints, poisoned(weights, np.inf, (n - 1, 0)), 3), "negative or not finite"),
        "skin: four zero weights": (lambda: a.set_mesh_skin(TUBE, joints, poisoned(weights, 0.0, (7, slice(None))), 3), "four zero weights"),
        "morph: bad index": (lambda: a.set_mesh_morph_targets(99, dp, dn), "bad mesh index"),
        "morph: isosurface mesh": (lambda: a.set_mesh_morph_targets(iso, np.zeros((1, 3, 3), np.float32)), "isosurface"),
        "morph: wrong count": (lambda: a.set_mesh_morph_targets(TUBE, dp[:, :-1], dn[:, :-1]), "vertex count"),
        "morph: no targets": (lambda: raw(morph, TUBE, dpp, None, n, 0), "num_targets"),
        "morph: null deltas": (lambda: raw(morph, TUBE, None, None, n, 3), "null"),
        "morph: NaN position delta": (lambda: a.set_mesh_morph_targets(TUBE, poisoned(dp, np.nan, (2, n - 1, 2)), dn), "delta is not finite"),
        "morph: inf normal delta": (lambda: a.set_mesh_morph_targets(TUBE, dp, poisoned(dn, -np.inf, (0, 0, 0))), "delta is not finite"),
        "pose: bad index": (lambda: a.pose_mesh(99, jm, mw), "bad mesh index"),
        "pose: isosurface mesh": (lambda: a.pose_mesh(iso, jm, mw), "isosurface"),
        "pose: neither part": (lambda: a.pose_mesh(BOX, jm, mw), "neither"),
        "pose: wrong joint count": (lambda: a.pose_mesh(TUBE, jm[:2], mw), "num_joints"),
        "pose: no matrices": (lambda: a.pose_mesh(TUBE, None, mw), "num_joints"),
        "pose: null matrices": (lambda: raw(pose, TUBE, None, 3, mwp, 3), "num_joints"),
        "pose: wrong target count": (lambda: a.pose_mesh(TUBE, jm, mw[:2]), "num_targets"),
        "pose: no weights": (lambda: a.pose_mesh(TUBE, jm, None), "num_targets"),
        "pose: null weights": (lambda: raw(pose, TUBE, jmp, 3, None, 3), "num_targets"),
        "pose: NaN matrix": (lambda: a.pose_mesh(TUBE, poisoned(jm, np.nan, (2, 11)), mw), "joint matrix is not finite"),
        "pose: inf matrix": (lambda: a.pose_mesh(TUBE, poisoned(jm, np.inf, (0, 0)), mw), "joint matrix is not finite"),
        "pose: NaN morph weight": (lambda: a.pose_mesh(TUBE, jm, poisoned(mw, np.nan, 1)), "morph weight is not finite"),
    }
    poses, updates = a.pose_stats().poses, a.mesh_update_stats().updates
    for name, (call, match) in cases.items():
        refused(call, match)
        assert match.split()[0] in lib.uh_last_error(ctx).decode(), name
    for fn, args in ((skin, (TUBE, jp, wp, n, 3)), (morph, (TUBE, dpp, None, n, 3)), (pose, (TUBE, jmp, 3, mwp, 3))):
        assert fn(None, *args) == 1, "a null context"
    assert lib.uh_get_pose_stats(None, None) == 1
    # nothing was stored, nothing moved: still built, the same answers, and the rig is the one set before the refusals
    md.assert_same(md.traced(a), before, "traces after the refusals")
    assert (a.pose_stats().poses, a.mesh_update_stats().updates) == (poses, updates)
    assert_bits(a.read_mesh(TUBE)[0], tube_posed(0), "the tube after the refusals")
    pose_tube(a, 1)
    assert_bits(a.read_mesh(TUBE)[0], tube_posed(1), "the tube posed after the refusals")


# ---- 5. the set verbs, the stats -----------------------------------------------------------------------------------------------------------
def test_the_set_verbs_leave_a_built_context_built_and_take_the_current_vertices():
    a = make_ctx(tube()[0], 1)
    before = md.traced(a)
    rig(a)
    md.assert_same(md.traced(a), before, "traces after the set verbs: no build, no refit between")
    v, _, joints, weights, dp, dn = tube()
    pose_tube(a, 0)
    # set again: the posed vertices (on the device; the host copy is stale) are the new bind pose
    a.set_mesh_skin(TUBE, joints, weights, TUBE_JOINTS)
    jm = tube_pose(2)[0]
    a.pose_mesh(TUBE, jm, np.zeros(TUBE_TARGETS, np.float32))
    twice = ref.pose(tube_posed(0), joints, weights, jm)
    assert_bits(a.read_mesh(TUBE)[0], twice, "a pose of the posed tube")
    # after a host update the host copy is the bind pose; a later update leaves the bind pose alone
    a.update_mesh_vertices(TUBE, v)
    a.set_mesh_morph_targets(TUBE, dp[:1])
    a.update_mesh_vertices(TUBE, tube_posed(1))
    a.pose_mesh(TUBE, jm, np.float32([0.5]))
    assert_bits(a.read_mesh(TUBE)[0], ref.pose(v, joints, weights, jm, dp[:1], None, np.float32([0.5])), "a pose from the re-set bind pose")
    a.rebuild_tlas()
    md.assert_sound(a)


def test_stats_are_zero_before_the_first_pose_and_counted_after_it():
    a = make_ctx(tube()[0], 1, rigged=True)
    s = a.pose_stats()
    assert bytes(s) == bytes(32), "all zero before the first pose"
    assert bytes(a.mesh_update_stats()) == bytes(32)
    nv = len(tube()[0])
    for k in range(3):
        pose_tube(a, k)
        a.rebuild_tlas()
    s, u = a.pose_stats(), a.mesh_update_stats()
    assert (s.poses, s.vertices, s.joints, s.active_targets, s.staged_joint_limit) == (3, nv, TUBE_JOINTS, 2, STAGED_LIMIT)
    assert s.pose_ms > 0.0
    params = 48 * TUBE_JOINTS + 8 * 2
    assert s.device_bytes == 2 * 80 * nv + 24 * nv + 24 * TUBE_TARGETS * nv + params + 4
    assert u.updates == 3 and u.host_geometry_bytes == 0, "poses and refits moved geometry through the host"
    assert u.device_bytes == 80 * nv + 4 * len(tube()[1])

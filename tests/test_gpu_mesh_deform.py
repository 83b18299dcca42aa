"""GPU: uh_update_mesh_vertices - new vertices for a mesh of uh_add_mesh, its index list and the tree's topology kept, served by a refit
on the device (k_deform_gather, then refit.hip) or by a build. The verb is defined by equivalence: after the update and either way
out, every observable of the context (the mesh itself, traces, path-traced frames with both grids, the cast and the rasterised
G-buffer, the shadow maps, the forward graph) equals, bit for bit, that of a fresh context made with uh_add_mesh from the new vertices
and built - for every builder, for host and for device input. Phase 1 of the deforming sheet lies wholly outside the box of phase 0:
boxes left stale would lose hits."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Scene, box, icosphere, quad
from rust_renderer_amd.types import RESERVOIR_DTYPE, VERTEX_DTYPE
from util import DeviceBuffer, random_rays

pytestmark = pytest.mark.gpu
W, H = 96, 64
LIGHTS = [(6.0, 30.0, 6.0), (28.0, 12.0, 30.0), (16.0, 34.0, 16.0)]
GROUND, SPHERE, DEFORM, BOX = range(4)  # the deforming mesh is neither first nor last
RAY_BOUNDS = ((-2, 4, -2), (34, 34, 34))
MISS = 0xFFFFFFFF
GRID, SHEET, AMPLITUDE, LIFT = 24, 16.0, 3.0, 6.0
FX, FZ = 0.56, 0.28  # (chosen so that no vertex of the 25 x 25 grid comes within 2e-3 of a crest or a trough)
DEFORM_TRIS = 2 * GRID * GRID
T_HALF_PI = 5.2359877  # the density field at this time crosses one cell of the 8^3 grid over [21.5, 24.5]^3: a one-triangle isosurface


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    mx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    my = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    mz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (mz @ my @ mx).astype(np.float32)


DEFORM_WORLD = rr.transform3x4((1.05, 0.9, 1.1), (15.0, 10.0, 15.0), _rot(0.15, 0.5, -0.1))
SPHERE_WORLD = rr.transform3x4((3, 3, 3), (4.0, 9.0, 26.0))


@functools.lru_cache(maxsize=None)
def _sheet():
    v, idx = quad((-SHEET / 2, 0.0, -SHEET / 2), (0, 0, SHEET), (SHEET, 0, 0), GRID, GRID)
    assert len(v) == (GRID + 1) ** 2 and len(idx) == 3 * DEFORM_TRIS, "the sheet's vertices are not shared"
    for a in (v, idx):
        a.setflags(write=False)
    return v, idx


@functools.lru_cache(maxsize=None)
def phase(k):
    """the sheet at phase k: y = AMPLITUDE sin(FX x + FZ z + 0.9 k), phase 1 lifted by LIFT; normals from the analytic gradient, uvs
    shifted by 0.1 k. Phase 0 is not the flat quad either"""
    v = _sheet()[0].copy()
    x, z = v["pos"][:, 0].astype(np.float64), v["pos"][:, 2].astype(np.float64)
    arg = FX * x + FZ * z + 0.9 * k
    v["pos"][:, 1] = AMPLITUDE * np.sin(arg) + (LIFT if k == 1 else 0.0)
    n = np.stack([-AMPLITUDE * FX * np.cos(arg), np.ones_like(arg), -AMPLITUDE * FZ * np.cos(arg)], axis=1)
    v["normal"][:, :3] = n / np.linalg.norm(n, axis=1, keepdims=True)
    v["uv"] = _sheet()[0]["uv"] + np.float32(0.1 * k)
    v.setflags(write=False)
    return v


def camera():
    return Camera((27.0, 19.0, 33.0), (16.0, 14.0, 16.0), 60.0, W / H, 0.01, 1000.0)


def make_view(rebuild_tlas=0):
    v = Scene("deform", [], LIGHTS, camera(), {}).make_view(W, H)
    v.rebuild_tlas = rebuild_tlas
    return v


def fill_scene(r, k, deform_world=DEFORM_WORLD, sphere_world=SPHERE_WORLD, extra=()):
    """ground, sphere, the sheet at phase k, box, three lights; `extra`: (vertices, indices, world) meshes behind them. Not built"""
    def mat(*rgb):
        return rr.make_material(base_color=rgb + (1.0,), diffuse_map=r.default_diffuse_map())

    assert r.add_mesh(*quad((-64, 4.99, -64), (0, 0, 160), (160, 0, 0), 8, 8), mat(0.6, 0.6, 0.6)) == GROUND
    assert r.add_mesh(*icosphere(2), mat(0.8, 0.3, 0.2), sphere_world) == SPHERE
    assert r.add_mesh(phase(k), _sheet()[1], mat(0.8, 0.8, 0.8), deform_world) == DEFORM
    assert r.add_mesh(*box((27.0, 7.5, 8.0), (2.0, 2.5, 2.0)), mat(0.2, 0.4, 0.8)) == BOX
    for v, idx, world in extra:
        r.add_mesh(v, idx, mat(0.3, 0.8, 0.4), world)
    for p in LIGHTS:
        r.add_light(p, (1.0, 0.9, 0.8), 40.0)
    return r


def make_ctx(k, device_build, **scene):
    r = rr.Renderer(W, H)
    r.set_option("sun_grid_force", 1)  # the sun grid refuses scenes with a ground plane by default
    r.set_option("device_build", device_build)
    fill_scene(r, k, **scene)
    r.build_acceleration()
    return r


def device_copy(vertices):
    """the vertices in a plain device allocation, as a caller's own HIP code would hold them"""
    vertices = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
    buf = DeviceBuffer(vertices.nbytes)
    assert buf.hip().hipMemcpy(buf.ptr, vertices.ctypes.data, vertices.nbytes, 1) == 0  # hipMemcpyHostToDevice
    assert buf.hip().hipDeviceSynchronize() == 0
    return buf


def update(r, vertices, where, mesh=DEFORM):
    if where == "host":
        r.update_mesh_vertices(mesh, vertices)
        return
    buf = device_copy(vertices)
    r.update_mesh_vertices(mesh, device_ptr=buf.ptr, count=len(vertices))
    buf.zero(0, buf.nbytes)  # the caller may reuse its buffer after return: the library must have taken a copy
    buf.free()


def way_out(r, how):
    r.rebuild_tlas() if how == "refit" else r.build_acceleration()


def frames(r, n=3, mask=rr.PASS_ALL, rebuild_tlas=0):
    """n frames of a camera at rest from cleared temporal state and a view of its own"""
    r.reset_accumulation()
    for which in range(3):
        r.write_reservoirs(which, np.zeros((r.height, r.width), dtype=RESERVOIR_DTYPE))
    loop = rr.FrameLoop(r, make_view(rebuild_tlas))
    for _ in range(n):
        loop.frame(mask)
    return loop


def traced(r, rays=None):
    rays = random_rays(RAY_BOUNDS, 30000, seed=7) if rays is None else rays
    tuv, mesh, prim = r.trace_closest(rays)
    return dict(tuv=tuv.view(np.uint32), mesh=mesh, prim=prim, any=r.trace_any(rays))


def path_traced(r, rebuild_tlas=0):
    r.reset_stats()
    frames(r, rebuild_tlas=rebuild_tlas)
    s = r.get_stats()
    return dict(acc=r.read_accumulation().view(np.uint32), rays=np.array(list(s.rays)), bvh_triangles=np.array(s.bvh_triangles)), s


def one_raster(r, rebuild_tlas=0):
    v = make_view(rebuild_tlas)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    r.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER)
    return dict(gbuffer_depth=r.read_hybrid(rr.HYBRID_GBUFFER_DEPTH), gbuffer_visibility=r.read_hybrid(rr.HYBRID_GBUFFER_VISIBILITY))


def forwarded(r, rebuild_tlas=0):
    v = make_view(rebuild_tlas)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    r.render_forward(v, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    return dict(forward_output=r.read_forward(rr.FORWARD_OUTPUT), forward_depth=r.read_forward(rr.FORWARD_DEPTH),
                forward_visibility=r.read_forward(rr.FORWARD_VISIBILITY))


def rastered(r):
    v = make_view()
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    out = {}
    r.render_hybrid(v, rr.HYBRID_GBUFFER)
    for name, k in (("position", rr.HYBRID_POSITION), ("normal", rr.HYBRID_NORMAL), ("albedo", rr.HYBRID_ALBEDO), ("pbr", rr.HYBRID_PBR)):
        out["cast_" + name] = r.read_hybrid(k)
    out.update(one_raster(r))
    r.set_option("shadow_map_size", 128)
    r.set_shadowmap_params(rr.shadow_cascades(camera(), v.sun_dir[:]))
    v.shadows_enabled = 1
    r.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    for c in range(4):
        out[f"shadow_map_{c}"] = r.read_shadow_map(c)
    out.update(forwarded(r))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differs in {np.count_nonzero(x != y) if x.shape == y.shape else 'shape'}"


def assert_same_mesh(a, b, mesh=DEFORM):
    (va, ia), (vb, ib) = a.read_mesh(mesh), b.read_mesh(mesh)
    assert va.tobytes() == vb.tobytes(), "not all 80 bytes of every vertex are the fresh mesh's"
    assert np.array_equal(ia, ib)


def assert_sound(r):
    rep = r.check_acceleration()
    assert rep["violations"] == dict.fromkeys(rep["violations"], 0) and rep["first"] == "" and rep["geometry_checked"], rep["first"]


def assert_grids(s):
    assert s.sun_grid_cells > 0 and s.camera_grid_cells > 0, "a grid was refused: its invalidation would go untested"


def deform_draw_range():
    first = 128 + 320
    return first, first + DEFORM_TRIS


def _refused(call, name):
    with pytest.raises(UtopianError, match=name):
        call()


def test_the_phases_are_what_the_tests_below_rely_on():
    p0, p1 = phase(0), phase(1)
    # the padded box of phase 0 (refit.hip: 1e-4 + 1e-5 |x|) ends below every vertex of phase 1, in object space and therefore under
    # the instance's transform
    assert p1["pos"][:, 1].min() > p0["pos"][:, 1].max() + 1e-3
    for a, b in ((0, 1), (1, 2), (2, 3)):
        for field in ("pos", "normal", "uv"):
            assert not np.array_equal(phase(a)[field], phase(b)[field]), field
    assert np.allclose(np.linalg.norm(p1["normal"][:, :3], axis=1), 1.0, atol=1e-6)


# ---- 1. equivalence: every builder, host and device input, both ways out -----------------------------------------------------------
@pytest.mark.parametrize("how", ["refit", "build"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("device_build", [0, 1, 2])
def test_update_equals_a_fresh_context(device_build, where, how):
    a = make_ctx(0, device_build)
    before = traced(a)
    _, s = path_traced(a)  # both grids and, below, the raster tables settle on the old geometry
    assert_grids(s)
    old = rastered(a)
    bytes_before = a.mesh_update_stats().host_geometry_bytes
    update(a, phase(1), where)
    way_out(a, how)
    if where == "device" and device_build in (1, 2):
        assert a.mesh_update_stats().host_geometry_bytes == bytes_before, "the device route moved geometry through the host"
    assert_sound(a)
    b = make_ctx(1, device_build)
    ta, tb = traced(a), traced(b)
    assert_same(ta, tb, "traces")
    assert np.count_nonzero(ta["mesh"] == DEFORM) > 500 and not np.array_equal(ta["tuv"], before["tuv"])
    (pa, sa), (pb, sb) = path_traced(a), path_traced(b)
    assert_same(pa, pb, "frames")
    assert_grids(sa), assert_grids(sb)
    assert pa["bvh_triangles"] == 128 + 320 + DEFORM_TRIS + 12
    ra = rastered(a)
    assert_same(ra, rastered(b), "raster")
    lo, hi = deform_draw_range()
    for k in ("gbuffer_visibility", "forward_visibility"):
        assert np.count_nonzero((ra[k] >= lo) & (ra[k] < hi)) > 50, k
    for k in ("cast_position", "cast_normal", "gbuffer_depth", "forward_depth", "forward_output"):
        assert not np.array_equal(bits(ra[k]), bits(old[k])), f"{k}: the update changed nothing"
    assert_same_mesh(a, b)
    assert a.read_mesh(DEFORM)[0].tobytes() == phase(1).tobytes()


# ---- 2. aimed rays against brute force ----------------------------------------------------------------------------------------------
def _world(p, m=DEFORM_WORLD):
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


@functools.lru_cache(maxsize=None)
def _aimed():
    """2,000 rays from above the sheet at points of its phase-1 triangles in world space - a third inside a triangle, a third on an
    edge, a third at a vertex, so that a box a step too small shows - and the oracle's brute-force answers: once, never written to"""
    n = 2000
    rng = np.random.default_rng(77)
    tris = phase(1)["pos"][:, :3][_sheet()[1].reshape(-1, 3)].astype(np.float64)  # (triangles, 3 vertices, 3)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    k = np.arange(n) % 3
    w[k == 1, 2] = 0.0
    w[k == 1] /= w[k == 1].sum(axis=1, keepdims=True)
    w[k == 2] = np.eye(3)[rng.integers(0, 3, int((k == 2).sum()))]
    target = _world(np.einsum("rv,rva->ra", w, tris[rng.integers(0, len(tris), n)])).astype(np.float32)
    above = np.stack([rng.uniform(-12, 12, n), rng.uniform(15, 30, n), rng.uniform(-12, 12, n)], axis=1)  # object space: over every crest
    origin = _world(above).astype(np.float32)
    rays = np.empty((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 0.001, target - origin, 10000.0
    cpu = fill_scene(oa.OracleRenderer(8, 8, brute_force=True), 1)
    cpu.build_acceleration()
    tuv, mesh, prim = cpu.trace_closest(rays)
    occluded = cpu.trace_any(rays)
    for a in (rays, tuv, mesh, prim, occluded):
        a.setflags(write=False)
    return rays, tuv, mesh, prim, occluded


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("builder", [(1, 0), 2], ids=str)
def test_aimed_rays_after_a_refit_equal_brute_force(builder, where):
    rays, tuv, mesh, prim, occluded = _aimed()
    assert (mesh == DEFORM).mean() > 0.5, "the rays must hit the sheet they are aimed at"
    kind, top = builder if isinstance(builder, tuple) else (builder, None)
    r = rr.Renderer(16, 16)
    r.set_option("device_build", kind)
    if top is not None:
        r.set_option("ploc_sah_top", top)
    fill_scene(r, 0)
    r.build_acceleration()
    update(r, phase(1), where)
    r.rebuild_tlas()
    assert_sound(r)
    tg, mg, pg = r.trace_closest(rays)
    assert np.array_equal(mg, mesh) and np.array_equal(pg, prim)
    assert np.array_equal(tg.view(np.uint32), tuv.view(np.uint32)), "t / u / v must equal brute force bit for bit"
    assert np.array_equal(r.trace_any(rays), occluded)


# ---- 3. sequences -------------------------------------------------------------------------------------------------------------------
def assert_step(a, device_build, what, **scene):
    b = make_ctx(device_build=device_build, **scene)
    assert_same(traced(a), traced(b), f"{what}: traces")
    assert_same(one_raster(a), one_raster(b), f"{what}: raster")
    assert_sound(a)
    assert_same_mesh(a, b)


@pytest.mark.parametrize("device_build", [0, 1])
def test_sequences_of_updates_refits_and_moved_instances(device_build):
    a = make_ctx(0, device_build)
    frames(a, 1), one_raster(a)
    for k, where in ((1, "device"), (2, "host"), (3, "device")):
        update(a, phase(k), where)
        a.rebuild_tlas()
        assert_step(a, device_build, f"phase {k}", k=k)
        frames(a, 2)
    # instances moved between the update and the refit, the deforming one among them, are served by the one refit
    w_deform = rr.transform3x4((0.9, 1.1, 1.0), (17.0, 11.0, 13.0), _rot(-0.1, 0.2, 0.25))
    w_sphere = rr.transform3x4((2.5, 3.5, 3.0), (6.0, 10.0, 24.0), _rot(0.3, 0.0, 0.1))
    update(a, phase(2), "device")
    a.set_instance_transform(DEFORM, w_deform)
    a.set_instance_transform(SPHERE, w_sphere)
    a.rebuild_tlas()
    assert_step(a, device_build, "phase 2 under moved instances", k=2, deform_world=w_deform, sphere_world=w_sphere)
    a.set_instance_transform(DEFORM, DEFORM_WORLD)
    a.set_instance_transform(SPHERE, SPHERE_WORLD)
    # a phase, a refit, the same phase again
    for where in ("host", "device"):
        update(a, phase(1), where)
        a.rebuild_tlas()
        assert_step(a, device_build, f"phase 1 ({where})", k=1)
    # phase 0 restored
    update(a, phase(0), "host")
    a.rebuild_tlas()
    assert_step(a, device_build, "phase 0 restored", k=0)
    b = make_ctx(0, device_build)
    assert_same(path_traced(a)[0], path_traced(b)[0], "frames at the end")
    assert_same(rastered(a), rastered(b), "raster at the end")


# ---- 4. view.rebuild_tlas, and meshes added since the build ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_the_graphs_refit_by_themselves_only_with_rebuild_tlas(where):
    a = make_ctx(0, 1)
    frames(a, 1), rastered(a)
    v, rays = make_view(), random_rays(RAY_BOUNDS, 64, seed=1)
    v.total_samples = 1
    update(a, phase(1), where)
    for call in (lambda: a.render_frame(v, rr.PASS_ALL), lambda: a.render_frames(v, rr.PASS_ALL, 2), lambda: a.render_hybrid(v, rr.HYBRID_GBUFFER),
                 lambda: a.render_forward(v, rr.FORWARD_PASS), lambda: a.trace_closest(rays), lambda: a.trace_any(rays)):
        _refused(call, "NOT_BUILT")
    assert_same(path_traced(a, rebuild_tlas=1)[0], path_traced(make_ctx(1, 1), rebuild_tlas=1)[0], "render_frame with rebuild_tlas")
    assert_sound(a)
    update(a, phase(2), where)
    assert_same(one_raster(a, rebuild_tlas=1), one_raster(make_ctx(2, 1)), "render_hybrid with rebuild_tlas")
    assert_sound(a)
    update(a, phase(3), where)
    assert_same(forwarded(a, rebuild_tlas=1), forwarded(make_ctx(3, 1)), "render_forward with rebuild_tlas")
    assert_sound(a)
    assert_same(traced(a), traced(make_ctx(3, 1)), "traces behind the three")


def test_a_mesh_added_since_the_build_needs_a_build():
    extra = (box((8.0, 12.0, 27.0), (1.5, 1.5, 1.5)) + (None,),)
    a = make_ctx(0, 1)
    a.add_mesh(extra[0][0], extra[0][1], rr.make_material(base_color=(0.3, 0.8, 0.4, 1.0), diffuse_map=a.default_diffuse_map()))
    update(a, phase(1), "device")
    _refused(a.rebuild_tlas, "NOT_BUILT")
    tlas = make_view(1)
    tlas.total_samples = 1
    _refused(lambda: a.render_frame(tlas, rr.PASS_ALL), "NOT_BUILT")
    a.build_acceleration()
    assert_sound(a)
    b = rr.Renderer(W, H)
    b.set_option("sun_grid_force", 1)
    b.set_option("device_build", 1)
    # (the lights come before the extra mesh in `a`, behind it in `b`: light and mesh tables do not depend on that order)
    fill_scene(b, 1, extra=extra).build_acceleration()
    assert_same(traced(a), traced(b), "traces")
    assert_same(one_raster(a), one_raster(b), "raster")


# ---- 5. two deforming meshes, one updated; a mesh without vertices -------------------------------------------------------------------
SECOND_WORLD = rr.transform3x4((0.5, 0.5, 0.5), (24.0, 16.0, 22.0), _rot(0.0, -0.4, 0.3))
SECOND, PLACEHOLDER = 4, 5


def _two_extra(k_second):
    return ((phase(k_second), _sheet()[1], SECOND_WORLD), (np.zeros(0, VERTEX_DTYPE), np.zeros(0, np.uint32), None))


@pytest.mark.parametrize("device_build", [0, 1])
def test_two_deforming_meshes_one_updated(device_build):
    a = make_ctx(0, device_build, extra=_two_extra(2))
    frames(a, 1), one_raster(a)
    second_before = a.read_mesh(SECOND)
    update(a, phase(1), "device")
    a.rebuild_tlas()
    s = a.mesh_update_stats()
    one_mesh = 80 * (GRID + 1) ** 2 + 4 * 3 * DEFORM_TRIS
    assert s.updates == 1 and s.triangles == DEFORM_TRIS and s.device_bytes == one_mesh, "the other sheet contributes to the stats"
    second = a.read_mesh(SECOND)
    assert second[0].tobytes() == second_before[0].tobytes() == phase(2).tobytes() and np.array_equal(second[1], second_before[1])
    assert_step(a, device_build, "the first sheet alone", k=1, extra=_two_extra(2))
    update(a, phase(3), "host", mesh=SECOND)
    a.rebuild_tlas()
    s = a.mesh_update_stats()
    assert s.updates == 2 and s.triangles == DEFORM_TRIS and s.device_bytes == 2 * one_mesh
    assert_step(a, device_build, "then the second", k=1, extra=_two_extra(3))
    assert a.read_mesh(SECOND)[0].tobytes() == phase(3).tobytes()
    # a mesh without vertices accepts a zero-count update, which changes nothing but the stats: the context stays built
    hits = traced(a)
    a.update_mesh_vertices(PLACEHOLDER, np.zeros(0, VERTEX_DTYPE))
    a.update_mesh_vertices(PLACEHOLDER, device_ptr=0, count=0)
    assert_same(traced(a), hits, "traces after the zero-count updates")
    s = a.mesh_update_stats()
    assert s.updates == 4 and s.triangles == DEFORM_TRIS and s.device_bytes == 2 * one_mesh
    assert tuple(len(x) for x in a.read_mesh(PLACEHOLDER)) == (0, 0)


# ---- 6. refusals leave everything as it was ------------------------------------------------------------------------------------------
def _poisoned(value, field=1):
    v = phase(1).copy()
    v["pos"][311, field] = value
    return v


@pytest.mark.parametrize("updated_before", [False, True], ids=["first_update", "after_an_update"])
def test_refused_updates_change_nothing(updated_before):
    a = rr.Renderer(W, H)
    a.set_option("sun_grid_force", 1)
    a.set_option("device_build", 1)
    fill_scene(a, 0)
    iso, tris = a.add_isosurface_mesh(8, 21.5, 24.5, T_HALF_PI)
    assert iso == 4 and tris == 1
    a.build_acceleration()
    if updated_before:
        update(a, phase(2), "device")
        a.rebuild_tlas()
    updates = a.mesh_update_stats().updates
    assert updates == (1 if updated_before else 0)
    frames(a, 2)
    before = a.read_accumulation().view(np.uint32)
    rays = random_rays(RAY_BOUNDS, 2000, seed=2)
    hits = traced(a, rays)
    mesh_before = a.read_mesh(DEFORM)[0].tobytes()
    fn = a._lib.uh_update_mesh_vertices
    fn.argtypes, fn.restype = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int], C.c_int
    good = np.ascontiguousarray(phase(1))
    n = len(good)
    poison = [device_copy(_poisoned(x, f)) for x, f in ((np.nan, 0), (np.inf, 1), (-np.inf, 2))]
    ok = device_copy(good)
    refusals = {
        "wrong count (host)": lambda: a.update_mesh_vertices(DEFORM, good[:-1]),
        "wrong count (device)": lambda: a.update_mesh_vertices(DEFORM, device_ptr=ok.ptr, count=n - 1),
        "zero count on a mesh with vertices": lambda: a.update_mesh_vertices(DEFORM, np.zeros(0, VERTEX_DTYPE)),
        "bad index": lambda: a.update_mesh_vertices(99, good),
        "isosurface mesh": lambda: a.update_mesh_vertices(iso, np.zeros(3, VERTEX_DTYPE)),
        "null host pointer": lambda: a._check(fn(a._ctx, DEFORM, None, n, 0)),
        "null device pointer": lambda: a.update_mesh_vertices(DEFORM, device_ptr=0, count=n),
        "where = 2": lambda: a._check(fn(a._ctx, DEFORM, good.ctypes.data, n, 2)),
        "where = -1": lambda: a._check(fn(a._ctx, DEFORM, good.ctypes.data, n, -1)),
        "NaN (host)": lambda: a.update_mesh_vertices(DEFORM, _poisoned(np.nan)),
        "inf (host)": lambda: a.update_mesh_vertices(DEFORM, _poisoned(np.inf, 2)),
        "NaN (device)": lambda: a.update_mesh_vertices(DEFORM, device_ptr=poison[0].ptr, count=n),
        "inf (device)": lambda: a.update_mesh_vertices(DEFORM, device_ptr=poison[1].ptr, count=n),
        "-inf (device)": lambda: a.update_mesh_vertices(DEFORM, device_ptr=poison[2].ptr, count=n),
    }
    for what, call in refusals.items():
        _refused(call, "INVALID_ARGUMENT")
        assert_same(traced(a, rays), hits, f"traces after the refused update: {what}")  # still built
        assert a.mesh_update_stats().updates == updates, what
    frames(a, 2)
    assert np.array_equal(a.read_accumulation().view(np.uint32), before)
    assert a.read_mesh(DEFORM)[0].tobytes() == mesh_before


# ---- 7. stats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_build", [0, 1])
def test_stats(device_build):
    a = make_ctx(0, device_build)
    assert bytes(a.mesh_update_stats()) == bytes(32), "the stats are not all zero before the first update"
    nv = (GRID + 1) ** 2
    update(a, phase(1), "host")
    s = a.mesh_update_stats()
    assert (s.updates, s.triangles, s.gather_ms, s.refit_ms) == (1, 0, 0.0, 0.0), "nothing has been refitted yet"
    assert s.host_geometry_bytes == 80 * nv and s.device_bytes == 80 * nv + 4 * 3 * DEFORM_TRIS
    a.rebuild_tlas()
    s = a.mesh_update_stats()
    assert s.updates == 1 and s.triangles == DEFORM_TRIS and s.gather_ms > 0.0 and s.refit_ms > 0.0 and s.device_bytes == 80 * nv + 4 * 3 * DEFORM_TRIS
    # the host builder's tree had no object-space corners on the device: the first refit uploads the sheet's from the host copy
    assert s.host_geometry_bytes == 80 * nv + (36 * DEFORM_TRIS if device_build == 0 else 0)
    moved = s.host_geometry_bytes
    for k in (2, 3):
        update(a, phase(k), "device")
        a.rebuild_tlas()
    s = a.mesh_update_stats()
    assert s.updates == 3 and s.triangles == DEFORM_TRIS and s.host_geometry_bytes == moved, "device updates and refits moved geometry through the host"
    a.read_mesh(DEFORM)
    assert a.mesh_update_stats().host_geometry_bytes == moved + 80 * nv
    if device_build == 0:
        # the host builder reads the mesh back once per device-input update, then uploads its packets (48 + 64 bytes per triangle)
        a.build_acceleration(), a.build_acceleration()
        assert a.mesh_update_stats().host_geometry_bytes == moved + 2 * 80 * nv + 2 * (48 + 64) * DEFORM_TRIS

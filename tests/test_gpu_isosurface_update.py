"""GPU: uh_update_isosurface_mesh - the marching-cubes field at another time as an existing mesh's geometry, on the device. The verb is
defined by equivalence: after the update and a build, every observable of the context (the mesh itself, traces, path-traced frames
with both grids, the cast and the rasterised G-buffer, the shadow maps, the forward graph) equals, bit for bit, that of a fresh context
made with uh_add_isosurface_mesh at that time in the first place - for every builder, when the count grows, shrinks, stays or becomes
zero, with the meshes behind it shifting. Triangle counts come from the CPU oracle (oracle_api.marching_cubes), never from a constant."""
import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Scene, box, icosphere, quad
from rust_renderer_amd.types import RESERVOIR_DTYPE, VERTEX_DTYPE
from util import random_rays

pytestmark = pytest.mark.gpu
W, H = 96, 64
LO, HI = 0.0, 32.0
T_PI = 10.471975      # 0.3 t = pi in float32: the count of t = 0 with other vertices
T_HALF_PI = 5.2359877
LIGHTS = [(6.0, 30.0, 6.0), (28.0, 12.0, 30.0), (16.0, 34.0, 16.0)]
GROUND, SPHERE, ISO, BOX = range(4)  # mesh indices: two static meshes before the isosurface, one after it (its range shifts)
RAY_BOUNDS = ((-2, 4, -2), (34, 34, 34))


def camera():
    return Camera((27.0, 19.0, 33.0), (16.0, 14.0, 16.0), 60.0, W / H, 0.01, 1000.0)


def make_view():
    return Scene("update", [], LIGHTS, camera(), {}).make_view(W, H)


def oracle(res, time, lo=LO, hi=HI, positions=True):
    return oa.marching_cubes(res, lo, hi, time=time, order=0, positions=positions)


def fill_scene(r, add_iso, statics=True):
    """ground and sphere, the isosurface's mesh - add_iso(material) adds it and returns its index -, box, three lights; without `statics`
    that mesh alone. Not built"""
    def mat(*rgb):
        return rr.make_material(base_color=rgb + (1.0,), diffuse_map=r.default_diffuse_map())

    if statics:
        assert r.add_mesh(*quad((-64, 4.99, -64), (0, 0, 160), (160, 0, 0), 8, 8), mat(0.6, 0.6, 0.6)) == GROUND
        assert r.add_mesh(*icosphere(2), mat(0.8, 0.3, 0.2), rr.transform3x4((3, 3, 3), (4.0, 9.0, 26.0))) == SPHERE
    mesh = add_iso(mat(0.8, 0.8, 0.8))
    if statics:
        assert mesh == ISO
        assert r.add_mesh(*box((27.0, 7.5, 8.0), (2.0, 2.5, 2.0)), mat(0.2, 0.4, 0.8)) == BOX
        for p in LIGHTS:
            r.add_light(p, (1.0, 0.9, 0.8), 40.0)
    return r


def make_ctx(res, time, device_build, lo=LO, hi=HI, placeholder=False, world=None, width=W, height=H, statics=True):
    """the scene with the isosurface at `time` (or, placeholder, a mesh without vertices in its place), built"""
    r = rr.Renderer(width, height)
    r.set_option("sun_grid_force", 1)  # the sun grid refuses scenes with a ground plane by default
    r.set_option("device_build", device_build)

    def add_iso(material):
        if placeholder:
            return r.add_mesh(np.zeros(0, VERTEX_DTYPE), np.zeros(0, np.uint32), material, world)
        mesh, tris = r.add_isosurface_mesh(res, lo, hi, time, material=material, world3x4=world)
        assert tris == oracle(res, time, lo, hi, positions=False)["triangles"]
        return mesh

    fill_scene(r, add_iso, statics)
    r.build_acceleration()
    return r


def frames(r, n=3, mask=rr.PASS_ALL):
    """n frames of a camera at rest from cleared temporal state - the accumulation and the reservoirs' history, which the first
    frame's temporal pass would otherwise read - and a view of its own"""
    r.reset_accumulation()
    for which in range(3):
        r.write_reservoirs(which, np.zeros((r.height, r.width), dtype=RESERVOIR_DTYPE))
    loop = rr.FrameLoop(r, make_view())
    for _ in range(n):
        loop.frame(mask)
    return loop


def update(r, time, res, lo=LO, hi=HI, mesh=ISO):
    tris = r.update_isosurface_mesh(mesh, time)
    assert tris == oracle(res, time, lo, hi, positions=False)["triangles"]
    r.build_acceleration()
    return tris


def traced(r, rays=None):
    rays = random_rays(RAY_BOUNDS, 30000, seed=7) if rays is None else rays
    tuv, mesh, prim = r.trace_closest(rays)
    return dict(tuv=tuv.view(np.uint32), mesh=mesh, prim=prim, any=r.trace_any(rays))


def path_traced(r):
    r.reset_stats()
    frames(r)
    s = r.get_stats()
    return dict(acc=r.read_accumulation().view(np.uint32), rays=np.array(list(s.rays)), bvh_triangles=np.array(s.bvh_triangles)), s


def rastered(r):
    v = make_view()
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    out = {}
    r.render_hybrid(v, rr.HYBRID_GBUFFER)
    for name, k in (("position", rr.HYBRID_POSITION), ("normal", rr.HYBRID_NORMAL), ("albedo", rr.HYBRID_ALBEDO), ("pbr", rr.HYBRID_PBR)):
        out["cast_" + name] = r.read_hybrid(k)
    r.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER)
    out["gbuffer_depth"] = r.read_hybrid(rr.HYBRID_GBUFFER_DEPTH)
    out["gbuffer_visibility"] = r.read_hybrid(rr.HYBRID_GBUFFER_VISIBILITY)
    r.set_option("shadow_map_size", 128)
    r.set_shadowmap_params(rr.shadow_cascades(camera(), v.sun_dir[:]))
    v.shadows_enabled = 1
    r.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    v.shadows_enabled = 0
    for c in range(4):
        out[f"shadow_map_{c}"] = r.read_shadow_map(c)
    r.render_forward(v, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    out["forward_output"] = r.read_forward(rr.FORWARD_OUTPUT)
    out["forward_depth"] = r.read_forward(rr.FORWARD_DEPTH)
    out["forward_visibility"] = r.read_forward(rr.FORWARD_VISIBILITY)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differs in {np.count_nonzero(x != y) if x.shape == y.shape else 'shape'}"


def iso_draw_range(r):
    first = sum(len(r.read_mesh(m)[1]) // 3 for m in range(ISO))
    return first, first + len(r.read_mesh(ISO)[1]) // 3


def assert_raster_sees_the_isosurface(r, images):
    lo, hi = iso_draw_range(r)
    for k in ("gbuffer_visibility", "forward_visibility"):
        assert np.count_nonzero((images[k] >= lo) & (images[k] < hi)) > 50, k
    assert np.count_nonzero(images["cast_pbr"][..., 3] == ISO) > 50


def assert_grids(s):
    assert s.sun_grid_cells > 0 and s.camera_grid_cells > 0, "a grid was refused: its invalidation would go untested"


# ---- 1. the mesh itself against the oracle and against a fresh mesh --------------------------------------------------------------
@pytest.mark.parametrize("kind,res,t0,t1", [("grow", 32, 0.0, 3.0), ("shrink", 40, 3.0, 1.0), ("same_count", 32, 0.0, T_PI)])
def test_updated_mesh_is_the_oracles_and_the_fresh_meshs(kind, res, t0, t1):
    before, after = oracle(res, t0), oracle(res, t1)
    assert not np.array_equal(before["positions"], after["positions"]), "t0 and t1 give the same mesh"
    grow = after["triangles"] - before["triangles"]
    assert {"grow": grow > 0, "shrink": grow < 0, "same_count": grow == 0}[kind]
    gpu = make_ctx(res, t0, 1, statics=False)
    assert gpu.update_isosurface_mesh(0, t1) == after["triangles"]
    v, idx = gpu.read_mesh(0)
    assert len(v) == len(idx) == 3 * after["triangles"]
    assert np.array_equal(v["pos"][:, :3].reshape(-1, 3, 3).view(np.uint32), after["positions"].reshape(-1, 3, 3).view(np.uint32))
    assert np.array_equal(idx, np.arange(3 * after["triangles"], dtype=np.uint32))
    fresh_v, fresh_idx = make_ctx(res, t1, 1, statics=False).read_mesh(0)
    assert v.tobytes() == fresh_v.tobytes(), "not all 80 bytes of every vertex are the fresh mesh's"
    assert np.array_equal(idx, fresh_idx)
    s = gpu.isosurface_update_stats()
    assert s.updates == 1 and s.triangles == after["triangles"] and s.extract_ms > 0.0 and s.device_bytes >= 240 * after["triangles"]


# ---- 2. traces and path-traced frames against a fresh context, every builder -------------------------------------------------------
@pytest.mark.parametrize("device_build", [0, 1, 2])
def test_traces_and_frames_equal_a_fresh_context(device_build):
    res, t0, t1 = 32, 0.0, 3.0
    a = make_ctx(res, t0, device_build)
    before = traced(a)
    _, s = path_traced(a)
    assert_grids(s)
    update(a, t1, res)
    b = make_ctx(res, t1, device_build)
    ta, tb = traced(a), traced(b)
    assert_same(ta, tb, "traces")
    assert np.count_nonzero(ta["mesh"] == ISO) > 500 and np.count_nonzero(tb["mesh"] == ISO) > 500
    assert not np.array_equal(ta["tuv"], before["tuv"]), "the update changed no hit"
    (pa, sa), (pb, sb) = path_traced(a), path_traced(b)
    assert_same(pa, pb, "frames")
    assert_grids(sa), assert_grids(sb)
    assert pa["bvh_triangles"] == 128 + 320 + oracle(res, t1, positions=False)["triangles"] + 12


# ---- 3. the raster consumers ------------------------------------------------------------------------------------------------------
def test_raster_tables_after_an_update_that_keeps_the_count():
    """the tables are then refreshed in place (the two meshes differ in a few last bits only: this holds the path to the fresh
    context's images, it cannot show a stale table)"""
    res, t0, t1 = 32, 0.0, T_PI
    a = make_ctx(res, t0, 1)
    rastered(a)
    assert update(a, t1, res) == oracle(res, t0, positions=False)["triangles"]
    ra = rastered(a)
    assert_same(ra, rastered(make_ctx(res, t1, 1)), "raster")
    assert a.isosurface_update_stats().host_geometry_bytes == 0
    assert_raster_sees_the_isosurface(a, ra)


@pytest.mark.parametrize("device_build", [0, 1])
def test_raster_consumers_equal_a_fresh_context(device_build):
    res, t0, t1 = 32, 0.0, 3.0
    a = make_ctx(res, t0, device_build)
    old = rastered(a)  # both graphs have been used before the update: stale tables would show
    update(a, t1, res)
    b = make_ctx(res, t1, device_build)
    ra, rb = rastered(a), rastered(b)
    assert_same(ra, rb, "raster")
    assert_raster_sees_the_isosurface(a, ra), assert_raster_sees_the_isosurface(b, rb)
    for k in ("cast_position", "gbuffer_depth", "forward_depth"):
        assert not np.array_equal(bits(ra[k]), bits(old[k])), f"{k}: the update changed nothing"
    assert any(not np.array_equal(bits(ra[f"shadow_map_{c}"]), bits(old[f"shadow_map_{c}"])) for c in range(4)), "no cascade sees the isosurface"


# ---- 4. there and back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_build", [0, 1])
def test_there_and_back(device_build):
    res = 32
    a = make_ctx(res, 0.0, device_build)
    counts = []
    for t in (3.0, 1.0, 0.0):
        counts.append(update(a, t, res))
        traced(a), frames(a, 2), rastered(a)
    assert counts[0] > counts[1] > counts[2], "the count never shrinks: stale tails would not show"
    b = make_ctx(res, 0.0, device_build)
    assert_same(traced(a), traced(b), "traces")
    (pa, sa), (pb, sb) = path_traced(a), path_traced(b)
    assert_same(pa, pb, "frames")
    assert_grids(sa), assert_grids(sb)
    ra, rb = rastered(a), rastered(b)
    assert_same(ra, rb, "raster")
    assert_raster_sees_the_isosurface(a, ra)
    va, vb = a.read_mesh(ISO), b.read_mesh(ISO)
    assert va[0].tobytes() == vb[0].tobytes() and np.array_equal(va[1], vb[1])


# ---- 4b. two device-resident meshes with host-resident ones between and behind them ------------------------------------------------
TWO_GROUND, TWO_A, TWO_SPHERE, TWO_B, TWO_BOX = range(5)
TWO_B_WORLD = rr.transform3x4((0.4, 0.4, 0.4), (-2.0, 3.0, 14.0))  # B beside A (x 1.2 .. 7.6; A starts at x = 8), left of it on screen


def make_two(res, t_a, t_b, device_build):
    """ground, isosurface A at t_a, sphere, isosurface B at t_b, box: built"""
    r = rr.Renderer(W, H)
    r.set_option("sun_grid_force", 1)
    r.set_option("device_build", device_build)

    def mat(*rgb):
        return rr.make_material(base_color=rgb + (1.0,), diffuse_map=r.default_diffuse_map())

    assert r.add_mesh(*quad((-64, 4.99, -64), (0, 0, 160), (160, 0, 0), 8, 8), mat(0.6, 0.6, 0.6)) == TWO_GROUND
    assert r.add_isosurface_mesh(res, LO, HI, t_a, material=mat(0.8, 0.8, 0.8)) == (TWO_A, oracle(res, t_a, positions=False)["triangles"])
    assert r.add_mesh(*icosphere(2), mat(0.8, 0.3, 0.2), rr.transform3x4((3, 3, 3), (4.0, 9.0, 26.0))) == TWO_SPHERE
    assert r.add_isosurface_mesh(res, LO, HI, t_b, material=mat(0.3, 0.8, 0.4), world3x4=TWO_B_WORLD) == (TWO_B, oracle(res, t_b, positions=False)["triangles"])
    assert r.add_mesh(*box((27.0, 7.5, 8.0), (2.0, 2.5, 2.0)), mat(0.2, 0.4, 0.8)) == TWO_BOX
    for p in LIGHTS:
        r.add_light(p, (1.0, 0.9, 0.8), 40.0)
    r.build_acceleration()
    return r


def assert_two_equal_fresh(a, res, t_a, t_b, device_build, what):
    """traces, both meshes and the raster consumers of `a` against a context created at (t_a, t_b); returns that context"""
    b = make_two(res, t_a, t_b, device_build)
    ta = traced(a)
    assert_same(ta, traced(b), f"{what}: traces")
    for mesh in (TWO_A, TWO_B):
        assert np.count_nonzero(ta["mesh"] == mesh) > 50, f"{what}: rays miss mesh {mesh}"
        (va, ia), (vb, ib) = a.read_mesh(mesh), b.read_mesh(mesh)
        assert va.tobytes() == vb.tobytes() and np.array_equal(ia, ib), f"{what}: mesh {mesh}"
    ra = rastered(a)
    assert_same(ra, rastered(b), f"{what}: raster")
    first = np.cumsum([0] + [len(a.read_mesh(m)[1]) // 3 for m in range(5)])
    for mesh in (TWO_A, TWO_B):
        for k in ("gbuffer_visibility", "forward_visibility"):
            assert np.count_nonzero((ra[k] >= first[mesh]) & (ra[k] < first[mesh + 1])) > 50, f"{what}: {k} misses mesh {mesh}"
    return b


@pytest.mark.parametrize("device_build", [0, 1])
def test_two_device_meshes_between_host_meshes(device_build):
    """one mesh updated while the other device-resident one and the host-resident ones behind it move by device copy; then the
    other with the layout kept; then both before a single build"""
    res = 32
    count = {t: oracle(res, t, positions=False)["triangles"] for t in (0.0, 1.0, 3.0, T_PI)}
    assert count[3.0] != count[0.0] == count[T_PI] and count[1.0] != count[3.0]
    a = make_two(res, 0.0, 0.0, device_build)
    rastered(a)  # both graphs have been used before the first update: stale tables would show
    assert update(a, 3.0, res, mesh=TWO_A) == count[3.0]
    assert_two_equal_fresh(a, res, 3.0, 0.0, device_build, "A alone")
    assert update(a, T_PI, res, mesh=TWO_B) == count[T_PI]
    assert_two_equal_fresh(a, res, 3.0, T_PI, device_build, "B alone")
    assert a.update_isosurface_mesh(TWO_A, 1.0) == count[1.0]
    assert update(a, 3.0, res, mesh=TWO_B) == count[3.0]  # (builds)
    b = assert_two_equal_fresh(a, res, 1.0, 3.0, device_build, "both")
    (pa, sa), (pb, sb) = path_traced(a), path_traced(b)
    assert_same(pa, pb, "frames")
    assert_grids(sa), assert_grids(sb)
    assert pa["bvh_triangles"] == 128 + count[1.0] + 320 + count[3.0] + 12


# ---- 5. a mesh that becomes empty --------------------------------------------------------------------------------------------------
def _aimed_rays(tri, n=2000, seed=3):
    """rays from around the scene towards points inside one triangle"""
    u = rr.scenes.hash_floats(seed, 5 * n).reshape(n, 5)
    w = np.stack([1.0 - np.sqrt(u[:, 0]), np.sqrt(u[:, 0]) * (1.0 - u[:, 1]), np.sqrt(u[:, 0]) * u[:, 1]], axis=1).astype(np.float32)
    target = w @ tri.astype(np.float32)
    origin = (np.float32([16, 20, 16]) + (u[:, 2:5] * 2.0 - 1.0) * 14.0).astype(np.float32)
    rays = np.empty((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 0.001, target - origin, 10000.0
    return rays


@pytest.mark.parametrize("device_build", [0, 1])
def test_a_mesh_that_becomes_empty_keeps_its_index_and_comes_back(device_build):
    res, lo, hi = 8, 21.5, 24.5
    assert oracle(res, T_HALF_PI, lo, hi)["triangles"] == 1
    for t in (0.0, 3.0, 4.5):
        assert oracle(res, t, lo, hi)["triangles"] == 0
    a = make_ctx(res, T_HALF_PI, device_build, lo, hi)
    tri = a.read_mesh(ISO)[0]["pos"][:, :3]
    rays = np.concatenate([_aimed_rays(tri), random_rays(RAY_BOUNDS, 10000, seed=9)])
    full = traced(a, rays)
    assert np.count_nonzero(full["mesh"] == ISO) > 10, "no ray hits the lone triangle"
    full_frames, _ = path_traced(a)
    assert a.update_isosurface_mesh(ISO, 0.0) == 0
    v, idx = a.read_mesh(ISO)
    assert len(v) == 0 and len(idx) == 0
    a.build_acceleration()
    b = make_ctx(res, 0.0, device_build, lo, hi, placeholder=True)
    empty = traced(a, rays)
    assert_same(empty, traced(b, rays), "traces over the empty mesh")
    assert not (empty["mesh"] == ISO).any() and np.count_nonzero(empty["mesh"] == BOX) > 0
    assert_same(path_traced(a)[0], path_traced(b)[0], "frames over the empty mesh")
    assert_same(rastered(a), rastered(b), "raster over the empty mesh")
    assert a.get_stats().bvh_triangles == 128 + 320 + 12
    assert update(a, T_HALF_PI, res, lo, hi) == 1
    assert_same(traced(a, rays), full, "traces after the mesh came back")
    assert_same(path_traced(a)[0], full_frames, "frames after the mesh came back")


# ---- 6. state and errors -----------------------------------------------------------------------------------------------------------
def _refused(call, name):
    with pytest.raises(UtopianError, match=name):
        call()


def test_not_built_until_the_build():
    a = make_ctx(32, 0.0, 1)
    frames(a, 1), rastered(a)
    a.update_isosurface_mesh(ISO, 1.0)
    v, rays = make_view(), random_rays(RAY_BOUNDS, 64, seed=1)
    v.total_samples = 1
    tlas = make_view()
    tlas.total_samples, tlas.rebuild_tlas = 1, 1
    for call in (lambda: a.render_frame(v, rr.PASS_ALL), lambda: a.render_frames(v, rr.PASS_ALL, 2), lambda: a.render_hybrid(v, rr.HYBRID_GBUFFER),
                 lambda: a.render_forward(v, rr.FORWARD_PASS), lambda: a.trace_closest(rays), lambda: a.trace_any(rays), a.rebuild_tlas,
                 lambda: a.render_frame(tlas, rr.PASS_ALL), lambda: a.render_hybrid(tlas, rr.HYBRID_GBUFFER), lambda: a.render_forward(tlas, rr.FORWARD_PASS)):
        _refused(call, "NOT_BUILT")
    a.build_acceleration()
    frames(a, 1)


def test_refused_calls_change_nothing():
    a = make_ctx(32, 0.0, 1)
    frames(a, 2)
    before = a.read_accumulation().view(np.uint32)
    rays = random_rays(RAY_BOUNDS, 2000, seed=2)
    hits = traced(a, rays)
    for mesh, time in ((99, 0.0), (GROUND, 1.0), (BOX, 1.0), (ISO, float("nan")), (ISO, float("inf")), (ISO, -float("inf"))):
        _refused(lambda: a.update_isosurface_mesh(mesh, time), "INVALID_ARGUMENT")
        assert_same(traced(a, rays), hits, "traces after a refused update")  # still built
        frames(a, 2)
        assert np.array_equal(a.read_accumulation().view(np.uint32), before)
    assert a.isosurface_update_stats().updates == 0


@pytest.mark.parametrize("device_build", [0, 1])
def test_instance_transform_and_refit_on_an_updated_mesh(device_build):
    res, t1 = 32, 3.0
    w1 = rr.transform3x4((0.8, 0.9, 0.8), (3.0, 1.0, 2.0))
    w2 = rr.transform3x4((0.7, 0.8, 0.9), (4.0, 2.0, 1.0))
    a = make_ctx(res, 0.0, device_build)
    untouched = traced(a)
    a.update_isosurface_mesh(ISO, t1)
    a.set_instance_transform(ISO, w1)
    a.build_acceleration()
    b = make_ctx(res, t1, device_build, world=w1)
    ta = traced(a)
    assert_same(ta, traced(b), "traces under the transform")
    assert np.count_nonzero(ta["mesh"] == ISO) > 500 and not np.array_equal(ta["tuv"], untouched["tuv"])
    assert_same(path_traced(a)[0], path_traced(b)[0], "frames under the transform")
    for r in (a, b):
        r.set_instance_transform(ISO, w2)
        r.rebuild_tlas()
    tr = traced(a)
    assert_same(tr, traced(b), "traces after the refit")
    assert not np.array_equal(tr["tuv"], ta["tuv"])
    assert_same(path_traced(a)[0], path_traced(b)[0], "frames after the refit")
    assert_same(rastered(a), rastered(b), "raster after the refit")


# ---- 7. nothing crosses the host ---------------------------------------------------------------------------------------------------
def test_the_device_route_moves_no_geometry_through_the_host():
    res = 32
    a = make_ctx(res, 0.0, 1)
    z = a.isosurface_update_stats()
    assert bytes(z) == bytes(32), "the stats are not all zero before the first update"
    frames(a, 1), rastered(a)
    tris = 0
    for k, t in enumerate((1.0, 3.0, 2.0)):
        tris = update(a, t, res)
        frames(a, 1)
        v = make_view()
        v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
        a.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER)
        a.render_forward(v, rr.FORWARD_PASS)
        s = a.isosurface_update_stats()
        assert s.host_geometry_bytes == 0 and s.updates == k + 1 and s.triangles == tris
        assert s.extract_ms > 0.0 and s.scatter_ms > 0.0 and s.device_bytes >= 240 * tris
    nv, ni = (len(x) for x in a.read_mesh(ISO))
    assert nv == ni == 3 * tris
    assert a.isosurface_update_stats().host_geometry_bytes == 80 * nv + 4 * ni


def test_the_host_builder_reads_the_mesh_back_once_per_update():
    res = 32
    a = make_ctx(res, 0.0, 0)
    tris = a.update_isosurface_mesh(ISO, 3.0)
    assert a.isosurface_update_stats().host_geometry_bytes == 0
    a.build_acceleration()
    # the documented slow route: 80 bytes per vertex down, then the leaf-order triangle and shade packets up (48 + 64 bytes per triangle)
    per_build = (48 + 64) * tris
    assert a.isosurface_update_stats().host_geometry_bytes == 80 * 3 * tris + per_build
    a.build_acceleration()
    assert a.isosurface_update_stats().host_geometry_bytes == 80 * 3 * tris + 2 * per_build, "the mirror was read back twice"
    a.read_mesh(ISO)  # answered from the mirror
    assert a.isosurface_update_stats().host_geometry_bytes == 80 * 3 * tris + 2 * per_build


# ---- 8. full size -----------------------------------------------------------------------------------------------------------------
def test_full_size_update():
    """BASELINE.json configs[4]'s grid: 512^3, device_build = 1, t = 0 -> 3"""
    res = 512
    want = oracle(res, 3.0, positions=False)["triangles"]
    a = rr.Renderer(W, H)
    a.set_option("device_build", 1)
    mesh, tris0 = a.add_isosurface_mesh(res, LO, HI, 0.0)
    a.build_acceleration()
    rays = random_rays(RAY_BOUNDS, 30000, seed=11)
    before = traced(a, rays)
    assert a.update_isosurface_mesh(mesh, 3.0) == want != tris0
    a.build_acceleration()
    b = rr.Renderer(W, H)
    b.set_option("device_build", 1)
    assert b.add_isosurface_mesh(res, LO, HI, 3.0)[1] == want
    b.build_acceleration()
    ta = traced(a, rays)
    assert_same(ta, traced(b, rays), "traces at 512^3")
    assert np.count_nonzero(ta["mesh"] == mesh) > 1000 and not np.array_equal(ta["tuv"], before["tuv"])
    s = a.isosurface_update_stats()
    assert s.triangles == want == a.get_stats().bvh_triangles and s.host_geometry_bytes == 0

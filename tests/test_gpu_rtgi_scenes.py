"""GPU: one-bounce ray-traced diffuse GI (UH_HYBRID_RTGI) against the restatement of tests/rtgi_reference.py on scenes the pass had not
seen: the synthetic scene (a metal, normal-mapped floor, rotated and non-uniformly scaled instances, metallic-roughness and occlusion
maps, a metal sphere), the turned scene (back faces, a mirrored instance, metal, dielectric and type-4 hits, zero vertex normals, uv
outside [0, 1], a base colour that runs into every branch of the clamp), frame numbers that wrap in 32 bits, and geometry that changed
on the device between two frames (uh_update_mesh_vertices, uh_update_isosurface_mesh, a moved instance). tests/test_rtgi_cpu.py proves
the coverage counts asserted here on the restatement alone, on the oracle's G-buffer."""
import numpy as np
import pytest

import hybrid_reference as hr
import oracle_api as oa
import rtgi_reference as gi
import rust_renderer_amd as rr
import test_gpu_isosurface_update as iso
import test_gpu_mesh_deform as deform
from hybrid_util import bits, synthetic_scene
from rust_renderer_amd.scenes import Scene
from test_gpu_rtgi import World, integers, plain_deferred

pytestmark = pytest.mark.gpu

W, H = gi.W, gi.H
SETTINGS = [(3, 0), (3, 3), (16, 0), (16, 3)]  # (samples, blur_radius)


def table(meshes, key, material):
    """the composite's read of `key` for the G-buffer's material indices (rtgi_reference.composite: the defaults beyond the table)"""
    valid = material < len(meshes)
    default = dict(metallic=1.0, type=0.0)[key]
    return np.where(valid, np.array([m[key] for m in meshes], np.float32)[np.where(valid, material, 0)], np.float32(default))


# ---- B1: the synthetic scene ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    return World(synthetic_scene()), World(synthetic_scene())


@pytest.mark.parametrize("samples, blur_radius", SETTINGS)
def test_the_synthetic_scene(synthetic, samples, blur_radius):
    """metal pixels cast and keep their reflection (view.raytracing_supported = 1: the composite leaves them), the sphere's pixels carry
    metallic and occlusion texels that enter the composite, the G-buffer's normals come from normal maps, the instances at the hits are
    rotated and non-uniformly scaled, and rays meet all four meshes. Nearly every pixel has a missed ray, so this is also the largest
    set of pixels held to the sky's tolerance: measured on the MI355X, DESIGN.md section 2 "Ray-traced diffuse GI" """
    w, t = synthetic
    v = w.view()
    assert v.raytracing_supported == 1
    w.render(v, samples=samples, blur_radius=blur_radius)
    plain = plain_deferred(t, v)
    got = w.check(v, plain)
    g, cast = got["g"], got["cast"]
    material = g["pbr"][..., 3].astype(np.uint32)
    metal = (g["position"][..., 3] != 0) & (table(w.meshes, "type", material) == 1.0)
    assert metal.sum() >= 100 and cast[metal].all() and (got["radiance"][metal][:, 3] == 1).all() and got["radiance"][metal][:, :3].any()
    assert np.array_equal(bits(got["deferred"][metal]), bits(plain[metal])) and not got["touched"][metal].any()
    matte = cast & ~metal
    metallic = g["pbr"][..., 0] * table(w.meshes, "metallic", material)
    assert (matte & (metallic != 0)).sum() >= 20 and (matte & (g["pbr"][..., 2] != 1)).sum() >= 20
    assert got["touched"][matte].all() and (got["deferred"][matte][:, :3] != plain[matte][:, :3]).any()
    r = w.gathered(g, v)[4]
    assert all((r["mesh"] == i).sum() >= 10 for i in range(4)), "rays meet the floor, both spheres and the quad"
    assert r["flipped"].any()


# ---- B2, B3: the turned scene ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def turned():
    return World(gi.turned_scene()), World(gi.turned_scene())


def assert_turned_coverage(r, totals):
    """what tests/test_rtgi_cpu.py proves of the restatement on the oracle's G-buffer, here on the device's"""
    M, k = gi.TURNED_MESHES, r["kind"]
    flipped = r["flipped"]
    assert flipped.sum() >= 50 and (flipped & (k == gi.SUNLIT)).sum() >= 20 and (flipped & (r["mesh"] == M["wall"])).sum() >= 50
    for name in ("metal", "dielectric", "pbr", "mirrored"):
        assert (r["mesh"] == M[name]).sum() >= 20, name
    assert ((r["mesh"] == M["mirrored"]) & (k == gi.SUNLIT)).sum() >= 10
    zero = r["mesh"] == M["zero"]
    assert zero.sum() >= 10 and (k[zero] == gi.DARK).all() and not r["shadowed"][zero].any() and np.isnan(r["Nh"][zero]).all()
    assert totals[2] == (k == gi.SUNLIT).sum() + r["shadowed"].sum(), "the sun rays are those of the hits that face the sun: none from a NaN normal"
    clamp = (r["mesh"] == M["clamp"]) & (k == gi.SUNLIT)
    return clamp


@pytest.mark.parametrize("samples, blur_radius", SETTINGS)
def test_the_turned_scene(turned, samples, blur_radius):
    """B2 and B3 in one scene (rtgi_reference.turned_scene): World.check holds every ray's record through the pixel means bit for bit;
    the counts below say that the rays which need the turn, the mirrored instance, the odd materials, the zero normals and the clamp
    are there"""
    w, t = turned
    v = w.view()
    w.render(v, samples=samples, blur_radius=blur_radius)
    got = w.check(v, plain_deferred(t, v))
    counts, E, cast, totals, r = w.gathered(got["g"], v)
    clamp = assert_turned_coverage(r, totals)
    visible = np.unique(got["g"]["pbr"][..., 3][got["g"]["position"][..., 3] != 0])
    assert gi.TURNED_MESHES["zero"] not in visible and gi.TURNED_MESHES["clamp"] not in visible, "outside the camera's view"
    # the clamp: (negative, 3e38 / pi NdotL, NaN) is stored as (+0, max_radiance, +0)
    cap = np.float32(w.params["max_radiance"])
    assert clamp.sum() >= 10 and (r["L"][clamp] == (0.0, cap, 0.0)).all() and not np.signbit(r["L"][clamp]).any()
    assert np.isfinite(got["radiance"]).all() and not np.signbit(got["radiance"]).any()
    assert (got["counts"][..., gi.SUNLIT].reshape(-1)[r["rows"][clamp.any(axis=1)]] > 0).all(), "the device counted the clamped rays sunlit"


# ---- B4: frame numbers that wrap -------------------------------------------------------------------------------------------------
def test_frame_numbers_that_wrap_in_32_bits(turned):
    """the seed word is (frame * 64 + s) ^ SEED_XOR in 32 bits. total_samples = 2^26 + 8: frame * 64 wraps to 512; time = -0.0001:
    frameNumber is (uint)(int)(-1.0f) = 2^32 - 1 and frame * 64 = 0xFFFFFFC0. Both equal the restatement and differ from frame 0"""
    w, t = turned
    first = None
    for kw in (dict(), dict(total_samples=2 ** 26 + 8), dict(time=-0.0001)):
        v = w.view(**kw)
        frame = oa.frame_number(v)
        if kw:
            assert frame >= 2 ** 26 and (frame * 64) >= 2 ** 32
        if "time" in kw:
            assert frame == 2 ** 32 - 1
        w.render(v, samples=3, blur_radius=0)
        got = w.check(v, plain_deferred(t, v))
        if first is None:
            assert frame == 0
            first = got
        else:
            assert not np.array_equal(got["counts"], first["counts"]) and not np.array_equal(bits(got["radiance"]), bits(first["radiance"]))


# ---- C: after the geometry changed on the device -------------------------------------------------------------------------------
class Filled(Scene):
    """a scene whose meshes a function adds (fill(renderer): the fixtures of test_gpu_mesh_deform.py and test_gpu_isosurface_update.py)"""

    def __init__(self, name, fill, lights, camera):
        super().__init__(name, [], lights, camera)
        self.fill = fill

    def upload(self, renderer):
        self.fill(renderer)
        renderer.initialize_raytracing()
        return renderer


def on_the_oracle(world, scene):
    """the oracle and the mesh records of `world` replaced by `scene`'s: what the device holds after an update, built afresh"""
    cpu = oa.OracleRenderer(*world.size)
    world.set_oracle(cpu, hr.upload_recorded(scene, cpu, True))
    return world


def changed_world(scene):
    w, t = World(scene, deform.W, deform.H), World(scene, deform.W, deform.H)
    for x in (w, t):
        on_the_oracle(x, scene)  # (the mesh records of the oracle's upload: an isosurface reaches it through add_mesh)
    return w, t


def frame(w, t, v, samples=3, blur_radius=1):
    w.render(v, samples=samples, blur_radius=blur_radius)
    got = w.check(v, plain_deferred(t, v))
    return got, w.gathered(got["g"], v)[4]


def assert_the_change_shows(w, v, got, r, before, stale, mesh):
    """the frame after the change is not the frame before it, and the restatement of the geometry before the change (`stale`: its oracle
    and mesh records) on this frame's G-buffer differs from the device in counts and, on rays that meet `mesh` both times, in Nh"""
    assert not np.array_equal(got["counts"], before["counts"]) and not np.array_equal(bits(got["radiance"]), bits(before["radiance"]))
    cpu, meshes = stale
    counts, E, cast, totals, r_stale = gi.gather(cpu, meshes, got["g"], v, w.params)
    assert not np.array_equal(counts, got["counts"])
    both = (r["mesh"] == mesh) & (r_stale["mesh"] == mesh) & np.isfinite(r["Nh"]).all(axis=-1) & np.isfinite(r_stale["Nh"]).all(axis=-1)
    differ = both & (r["Nh"] != r_stale["Nh"]).any(axis=-1)
    print(f"{(r['mesh'] == mesh).sum()} rays meet mesh {mesh}; {both.sum()} also with the geometry before the change, {differ.sum()} of them with another Nh")
    assert (r["mesh"] == mesh).sum() >= 20 and differ.sum() >= 10


def deform_scene(k, **kw):
    return Filled("rtgi_deform", lambda r: deform.fill_scene(r, k, **kw), deform.LIGHTS, deform.camera())


def deform_view(w, **kw):
    v = w.view(**kw)
    v.num_lights = len(deform.LIGHTS)
    return v


@pytest.mark.parametrize("where", ["host", "device"])
def test_after_update_mesh_vertices(where):
    """C1: the rippled sheet of test_gpu_mesh_deform.py (25 x 25 vertices under a rotated, non-uniformly scaled instance) goes from
    phase 0 to phase 2 - positions and normals both change - between two frames of one context, with a refit"""
    w, t = changed_world(deform_scene(0))
    v = deform_view(w)
    before, _ = frame(w, t, v)
    stale = (w.cpu, w.meshes)
    for x in (w, t):
        deform.update(x.gpu, deform.phase(2), where)
        x.gpu.rebuild_tlas()
        on_the_oracle(x, deform_scene(2))
    got, r = frame(w, t, v)
    assert_the_change_shows(w, v, got, r, before, stale, deform.DEFORM)


MOVED_WORLD = rr.transform3x4((0.9, 1.1, 1.0), (14.0, 11.0, 16.0), deform._rot(-0.4, 1.3, 0.35))


def test_after_a_moved_instance_with_rebuild_tlas():
    """C3: the sheet's instance gets another rotation, scale and place; the next call carries view.rebuild_tlas = 1. A MeshShade that kept
    the old world matrix would give the old Nh"""
    w, t = changed_world(deform_scene(0))
    before, _ = frame(w, t, deform_view(w))
    stale = (w.cpu, w.meshes)
    for x in (w, t):
        x.gpu.set_instance_transform(deform.DEFORM, MOVED_WORLD)
        on_the_oracle(x, deform_scene(0, deform_world=MOVED_WORLD))
    v = deform_view(w, rebuild_tlas=1)
    got, r = frame(w, t, v)
    assert_the_change_shows(w, v, got, r, before, stale, deform.DEFORM)


ISO_RES = 32


class IsoScene(Scene):
    """the scene of test_gpu_isosurface_update.py: on the device the isosurface is extracted there (and read back); the oracle receives
    the triangles the device holds, as a mesh"""

    def __init__(self):
        super().__init__("rtgi_iso", [], iso.LIGHTS, iso.camera())
        self.held = None

    def upload(self, r):
        def add_iso(material):
            if r.backend == "hip":
                return r.add_isosurface_mesh(ISO_RES, iso.LO, iso.HI, 0.0, material=material)[0]
            return r.add_mesh(*self.held, material)

        iso.fill_scene(r, add_iso)
        r.initialize_raytracing()
        if r.backend == "hip":
            self.held = r.read_mesh(iso.ISO)
        return r


def test_after_update_isosurface_mesh():
    """C2: the isosurface of the 32^3 grid goes from time 0 to time 3 on the device - another triangle count, another topology - and the
    tree is built again"""
    sa, sb = IsoScene(), IsoScene()
    w, t = World(sa, iso.W, iso.H), World(sb, iso.W, iso.H)
    for x, s in ((w, sa), (t, sb)):
        on_the_oracle(x, s)
    v = w.view()
    v.num_lights = len(iso.LIGHTS)
    before, _ = frame(w, t, v)
    stale = (w.cpu, w.meshes)
    tris_before = len(sa.held[1]) // 3
    for x, s in ((w, sa), (t, sb)):
        iso.update(x.gpu, 3.0, ISO_RES)
        s.held = x.gpu.read_mesh(iso.ISO)
        on_the_oracle(x, s)
    assert len(sa.held[1]) // 3 != tris_before
    got, r = frame(w, t, v)
    assert_the_change_shows(w, v, got, r, before, stale, iso.ISO)

"""GPU: emissive meshes as area lights of the hybrid frame (uh_render_hybrid's UH_HYBRID_AREA_LIGHTS) against the restatement of
tests/area_light_reference.py on the device's own G-buffer and deferred output: the emitter table bit for bit for a host-built and both
device-built trees, the counts image byte for byte with the pass's totals, the two images and the composited deferred output within
hybrid_util.DEFERRED_ULP, determinism, geometry that changed on the device against a fresh context, a frame whose shadow rays make the
persistent walk refill, a scene without emitters, isolation, and the call with every neighbour."""
import numpy as np
import pytest

import area_light_reference as al
import rust_renderer_amd as rr
from hybrid_util import DEFERRED_ULP, bits, gbuf, pair, read_all, record, ulps
from rust_renderer_amd.types import VERTEX_DTYPE
from test_gpu_walk_chunks import LANES, one_block_per_cu
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

W, H = al.W, al.H
AREA = rr.HYBRID_AREA_LIGHTS
DIFFUSE, SPECULAR, COUNTS = rr.HYBRID_AREA_DIFFUSE, rr.HYBRID_AREA_SPECULAR, rr.HYBRID_AREA_COUNTS
OWN = (DIFFUSE, SPECULAR, COUNTS)
FRAME = rr.HYBRID_FRAME | AREA
LAMP_MESH = 3  # area_light_reference._room: floor, back wall, box, lamp


def integers(s):
    return (s.pixels, s.samples, s.shadow_rays, s.occluded, s.emitter_pixels)


class World:
    """a scene on a GPU renderer and on the oracle"""

    def __init__(self, scene, width=W, height=H, device_build=None):
        self.scene, self.size = scene, (width, height)
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        if device_build is not None:
            self.gpu.set_option("device_build", device_build)
            self.gpu.build_acceleration()
        self.params = al.default_params()

    def view(self, **kw):
        return al.scene_view(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        """a G-buffer pass first (rt_shadows reads the previous call's G-buffer: this camera's, whatever ran before), then the call"""
        self.params = al.default_params(**params)
        self.gpu.set_area_light_params(**self.params)
        self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        self.gpu.render_hybrid(v, mask)

    def own(self):
        return {i: self.gpu.read_hybrid(i) for i in OWN}

    def check(self, v, name, **params):
        """the frame without the bit (its deferred_output is what the pass adds to), then with it, against the restatement"""
        gpu = self.gpu
        self.render(v, rr.HYBRID_FRAME, **params)
        plain = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        self.render(v, FRAME, **params)
        g = gbuf(gpu)
        got = dict(counts=gpu.read_hybrid(COUNTS), diffuse=gpu.read_hybrid(DIFFUSE), specular=gpu.read_hybrid(SPECULAR), deferred=gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT))
        s = gpu.area_light_stats()
        want = al.image(self.cpu, self.meshes, g, v, self.params, plain)
        geo = g["position"][..., 3] != 0
        worst = {k: int(ulps(got[k][geo], want[k][geo]).max()) for k in ("diffuse", "specular", "deferred")}
        print(f"{name} {params}: totals {integers(s)} (want {want['totals']}); differing counts {(got['counts'] != want['counts']).any(axis=-1).sum()}; max ulp {worst}; "
              f"table {s.table_ms:.3f} sample {s.sample_ms:.3f} shadow {s.shadow_ms:.3f} filter {s.filter_ms:.3f} composite {s.composite_ms:.3f} ms")
        record("area_lights", name, **{f"{k}_max_ulp": u for k, u in worst.items()}, **{k: v_ for k, v_ in params.items()})
        assert got["counts"].dtype == np.uint8 and got["counts"].shape == (self.size[1], self.size[0], 4) and np.array_equal(got["counts"], want["counts"])
        assert integers(s) == want["totals"] and s.samples == s.pixels * self.params["samples"]
        assert s.emitters == len(want["table"]["keys"]) and s.total_weight == want["table"]["total"]
        assert s.sample_ms > 0 and s.shadow_ms > 0 and s.filter_ms > 0 and s.composite_ms > 0
        for k in ("diffuse", "specular"):
            assert got[k].dtype == np.float32 and np.isfinite(got[k]).all()
            assert np.array_equal(got[k][..., 3] == 1, want["cast"]) and not got[k][~want["cast"]].any(), k
            assert worst[k] <= DEFERRED_ULP, (k, worst[k])
        assert worst["deferred"] <= DEFERRED_ULP, worst
        assert np.array_equal(bits(got["deferred"][..., 3]), bits(plain[..., 3])), "alpha is untouched"
        if not self.params["show_emitters"]:
            assert np.array_equal(bits(got["deferred"])[want["emitter"]], bits(plain)[want["emitter"]]), "emitter pixels are left alone"
        return got, want


@pytest.fixture(scope="module")
def room():
    return World(al.room_scene())


@pytest.fixture(scope="module")
def three():
    return World(al.three_lamp_scene())


# ---- 1. the device against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_build", [0, 1, 2])
def test_table_equals_the_restatement_whatever_built_the_tree(device_build):
    w = World(al.three_lamp_scene(), device_build=device_build)
    w.render(w.view())
    keys, areas, weights = w.gpu.read_area_emitters()
    t = al.table(w.meshes)
    assert len(keys) == 6
    assert np.array_equal(keys, t["keys"]) and np.array_equal(bits(areas), bits(t["areas"])) and np.array_equal(weights, t["weights"])
    s = w.gpu.area_light_stats()
    assert (s.emitters, s.total_weight, s.table_builds) == (6, t["total"], 1) and s.table_ms > 0


@pytest.mark.parametrize("samples, blur_radius, show_emitters", [(1, 0, 1), (3, 1, 0), (16, 6, 1)])
def test_room_equals_the_restatement(room, samples, blur_radius, show_emitters):
    got, want = room.check(room.view(), "room", samples=samples, blur_radius=blur_radius, show_emitters=show_emitters)
    assert want["emitter"].sum() >= 10 and want["cast"].sum() > 1500
    if show_emitters:
        assert (got["deferred"][want["emitter"]][:, :3] == 1.0).all()
    lit, occ = got["counts"][..., al.LIT], got["counts"][..., al.OCCLUDED]
    assert lit.sum() > 0 and occ.sum() > 0 and got["counts"][..., al.AWAY].sum() > 0
    if samples > 1:
        assert ((lit > 0) & (occ > 0)).any(), "penumbra"


def test_three_lamps_equal_the_restatement(three):
    got, want = three.check(three.view(), "three_lamps", samples=16, blur_radius=3, intensity=0.5, max_weight=8.0, max_radiance=2.0)
    assert (got["deferred"][want["emitter"]][:, :3] == 0.5).all()
    picks = np.bincount(want["samples"]["pick"].reshape(-1), minlength=6)
    assert picks[3] == 0 and (np.delete(picks, 3) >= 1).all()


# ---- 2. determinism -------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_the_other_item_order_are_bit_identical(room):
    v = room.view()
    room.render(v, samples=5, blur_radius=2)
    first = {**room.own(), "d": room.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)}
    room.render(v, samples=5, blur_radius=2)
    second = {**room.own(), "d": room.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)}
    room.gpu.set_option("area_light_order", 1)
    try:
        room.render(v, samples=5, blur_radius=2)
        other = {**room.own(), "d": room.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)}
    finally:
        room.gpu.set_option("area_light_order", 0)
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k
        assert np.array_equal(first[k].view(np.uint8), other[k].view(np.uint8)), k
    with pytest.raises(rr.UtopianError, match="area_light_order"):
        room.gpu.set_option("area_light_order", 2)


# ---- 3. geometry that changed on the device ------------------------------------------------------------------------------------------
MOVED = rr.transform3x4((0.7, 1.0, 1.2), (0.8, -0.4, 0.5))


def _lamp_vertices(scale):
    from rust_renderer_amd.scenes import quad

    v, _ = quad(al.LAMP["origin"], al.LAMP["eu"], al.LAMP["ev"])
    v = v.copy()
    v["pos"][:, 0] *= np.float32(scale)
    v["pos"][:, 1] -= np.float32(0.5)
    return np.ascontiguousarray(v, dtype=VERTEX_DTYPE)


def _fresh(change):
    s = al.room_scene()
    lamp = s.models[0][0].meshes[LAMP_MESH]
    if change == "reshaped":
        lamp.vertices = _lamp_vertices(0.6)
    else:
        lamp.transform = MOVED
    return World(s)


@pytest.mark.parametrize("change", ["refit", "rebuild_tlas", "reshaped"])
def test_changed_geometry_equals_a_fresh_context(change):
    w = World(al.room_scene())
    v = w.view()
    p = dict(samples=4, blur_radius=2)
    w.render(v, **p)
    builds = w.gpu.area_light_stats().table_builds
    assert builds == 1
    for _ in range(3):
        w.render(v, **p)
    assert w.gpu.area_light_stats().table_builds == builds, "unchanged frames build nothing"
    before = w.own()
    if change == "reshaped":
        verts = _lamp_vertices(0.6)
        buf = DeviceBuffer(verts.nbytes)
        assert buf.hip().hipMemcpy(buf.ptr, verts.ctypes.data, verts.nbytes, 1) == 0 and buf.hip().hipDeviceSynchronize() == 0
        w.gpu.update_mesh_vertices(LAMP_MESH, device_ptr=buf.ptr, count=len(verts))
        buf.free()
        w.gpu.rebuild_tlas()
    else:
        w.gpu.set_instance_transform(LAMP_MESH, MOVED)
        if change == "refit":
            w.gpu.rebuild_tlas()
    moved_view = w.view()
    if change == "rebuild_tlas":
        # one call: the call that sets the bit carries rebuild_tlas = 1 with the refit pending, and its table must be the refitted tree's
        moved_view.rebuild_tlas = 1
        w.gpu.render_hybrid(moved_view, rr.HYBRID_GBUFFER | FRAME)
        assert w.gpu.area_light_stats().table_builds == builds + 1, "the build follows the refit inside the call"
        moved_view.rebuild_tlas = 0
    w.render(moved_view, **p)  # (a G-buffer call first, as the fresh context below renders: rt_shadows reads the previous G-buffer)
    assert w.gpu.area_light_stats().table_builds == builds + 1, "one build per change"
    fresh = _fresh(change)
    fresh.render(fresh.view(), **p)
    got, want = w.own(), fresh.own()
    assert any(not np.array_equal(before[i], got[i]) for i in OWN), "the change shows"
    for i in OWN:
        assert np.array_equal(got[i].view(np.uint8), want[i].view(np.uint8)), (change, i)
    assert np.array_equal(bits(w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), bits(fresh.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)))
    for a, b in zip(w.gpu.read_area_emitters(), fresh.gpu.read_area_emitters()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 4. a frame whose shadow rays refill the persistent walk --------------------------------------------------------------------------
def test_sixteen_samples_refill_the_walk():
    w = one_block_per_cu(World(al.room_scene(), 131, 97))
    got, want = w.check(w.view(), "room_131x97", samples=16, blur_radius=1)
    s = w.gpu.area_light_stats()
    assert s.shadow_rays > LANES, "more shadow rays than one static chunk of the grid: a wave refills"


# ---- 5. no emitters -------------------------------------------------------------------------------------------------------------------
def test_no_emitters_leave_the_frame_as_it_was():
    w = World(al.dark_scene())
    v = w.view()
    w.render(v, rr.HYBRID_FRAME)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v)
    assert np.array_equal(bits(w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), bits(plain))
    for i in OWN:
        assert not w.gpu.read_hybrid(i).any(), i
    s = w.gpu.area_light_stats()
    assert (s.pixels, s.samples, s.shadow_rays, s.emitter_pixels, s.emitters, s.total_weight) == (0, 0, 0, 0, 0, 0)
    keys, areas, weights = w.gpu.read_area_emitters()
    assert len(keys) == len(areas) == len(weights) == 0


# ---- 6. isolation ---------------------------------------------------------------------------------------------------------------------
def test_isolation_with_the_bit_clear(room):
    never = World(al.room_scene())
    v = room.view()
    mask = rr.HYBRID_FRAME | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY
    room.render(v, FRAME)  # this context has run the pass
    snaps = []
    for w in (room, never):
        w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        w.gpu.render_hybrid(v, mask)
        snaps.append({**read_all(w.gpu), **{i: w.gpu.read_hybrid(i) for i in (rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS, rr.HYBRID_GLOSSY_SCALE,
                                                                          rr.HYBRID_GLOSSY_BIAS, rr.HYBRID_GLOSSY_COUNTS)}})
    for i in snaps[0]:
        assert np.array_equal(snaps[0][i].view(np.uint8), snaps[1][i].view(np.uint8)), i
    with pytest.raises(ValueError, match="0..15"):
        never.gpu.read_hybrid(DIFFUSE)
    assert bytes(never.gpu.area_light_stats()) == bytes(88)


def _path_tracer_state(r):
    s = r.get_stats()
    out = dict(acc=bits(r.read_accumulation()), out=r.read_output_bgra8(), pos=bits(r.read_gbuffer_position()),
               stats=np.array(list(s.rays) + [s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses], np.uint64))
    for k in range(3):
        out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
    return out


def _neighbour_state(r):
    """the RTAO and RTGI passes' images and integer stats"""
    ao, g = r.rtao_stats(), r.rtgi_stats()
    return dict(ao_counts=r.read_hybrid(rr.HYBRID_AO_COUNTS), ssao=r.read_hybrid(rr.HYBRID_SSAO_IMAGE), gi_radiance=bits(r.read_hybrid(rr.HYBRID_GI_RADIANCE)),
                gi_counts=r.read_hybrid(rr.HYBRID_GI_COUNTS), ao_stats=np.array([ao.pixels, ao.rays, ao.occluded], np.uint64),
                gi_stats=np.array([g.pixels, g.rays, g.shadow_rays, g.misses], np.uint64))


def _lit_room():
    """the room with two point lights, so that the reservoir passes of the path-traced frames have something to hold"""
    s = al.room_scene()
    s.lights = [(0.0, 2.0, 1.0), (1.5, 1.0, 0.5)]
    return s


def test_the_bit_changes_no_reservoir_accumulation_gbuffer_position_stats_rtao_or_rtgi_state():
    w = World(_lit_room())
    loop = rr.FrameLoop(w.gpu, w.scene.make_view(W, H))
    for _ in range(3):
        loop.frame(rr.PASS_ALL)
    assert any(w.gpu.read_reservoirs(k).view(np.uint8).any() for k in range(3)), "the reservoirs hold data"
    v = w.view()
    mask = rr.HYBRID_FRAME | rr.HYBRID_RTAO | rr.HYBRID_RTGI
    w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    w.gpu.render_hybrid(v, mask)
    before, near_before, images_before = _path_tracer_state(w.gpu), _neighbour_state(w.gpu), read_all(w.gpu)
    assert near_before["ao_stats"][0] > 0 and near_before["ao_counts"].any() and near_before["gi_stats"][1] > 0, "the rtao and rtgi passes ran"
    w.gpu.set_area_light_params(samples=3)
    w.gpu.render_hybrid(v, mask | AREA)
    assert w.gpu.area_light_stats().shadow_rays > 0
    after, near_after, images_after = _path_tracer_state(w.gpu), _neighbour_state(w.gpu), read_all(w.gpu)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for k in near_before:
        assert np.array_equal(near_before[k], near_after[k]), k
    for i in range(9):
        same = np.array_equal(images_before[i].view(np.uint8), images_after[i].view(np.uint8))
        assert same == (i not in (rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_PRESENT_OUTPUT)), i


# ---- 7. with every neighbour ----------------------------------------------------------------------------------------------------------
def test_one_call_with_every_neighbour(three):
    """the pass's add is what stands between the deferred pass and the rtgi pass: deferred + add, from the read-back Df / Spf, equals what a
    call that stops there leaves; and the call with RTAO, RTGI, GLOSSY, GLASS, TAA and POST beside the bit runs and yields the same pass"""
    w = three
    v = w.view()
    base = rr.HYBRID_FRAME | rr.HYBRID_RTAO
    w.render(v, base, samples=3, blur_radius=2)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    ao = lambda: (w.gpu.read_hybrid(rr.HYBRID_AO_COUNTS), w.gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), (lambda s: (s.pixels, s.rays, s.occluded))(w.gpu.rtao_stats()))
    ao_plain = ao()
    assert ao_plain[2][0] > 0 and ao_plain[0].any(), "the rtao pass ran"
    w.render(v, base | AREA, samples=3, blur_radius=2)
    for a, b in zip(ao_plain, ao()):
        assert np.array_equal(a, b), "the rtao pass's counts, its ssao image and its stats are what they were"
    g = gbuf(w.gpu)
    own, after = w.own(), w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    tab = al.table(w.meshes)
    cast, emitter = al.classify(g, v, w.meshes, tab)
    want = al.composite(g, plain, own[DIFFUSE], own[SPECULAR], emitter.reshape(H, W), w.meshes, w.params)
    geo = g["position"][..., 3] != 0
    assert np.array_equal(own[DIFFUSE][..., 3] == 1, cast.reshape(H, W))
    u = int(ulps(after[geo], want[geo]).max())
    record("area_lights", "neighbours", composite_max_ulp=u)
    assert u <= DEFERRED_ULP
    w.render(v, base | AREA | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY | rr.HYBRID_GLASS | rr.HYBRID_TAA | rr.HYBRID_POST, samples=3, blur_radius=2)
    for i in OWN:
        assert np.array_equal(own[i].view(np.uint8), w.gpu.read_hybrid(i).view(np.uint8)), i
    for a, b in zip(ao_plain, ao()):
        assert np.array_equal(a, b), "and beside every neighbour"
    s = w.gpu.area_light_stats()
    assert s.pixels == cast.sum() and w.gpu.rtgi_stats().pixels > 0 and w.gpu.glossy_stats().pixels >= 0
    assert np.isfinite(w.gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT)).all()


# ---- 8. params refusals on a context ---------------------------------------------------------------------------------------------------
def test_a_refused_params_call_leaves_the_old_params(room):
    v = room.view()
    room.render(v, samples=2, blur_radius=1)
    before = room.own()
    bad = [("samples", 0), ("samples", 17), ("blur_radius", 7), ("show_emitters", 2), ("max_weight", 0.0), ("max_weight", float("inf")),
           ("max_radiance", float("nan")), ("max_radiance", -1.0), ("intensity", -1.0), ("intensity", float("inf")), ("blur_normal_cos", float("nan")),
           ("blur_plane", float("nan"))]
    for field, value in bad:
        with pytest.raises(rr.UtopianError, match=f"uh_set_area_light_params: .*{field}") as e:
            room.gpu.set_area_light_params(**al.default_params(**{field: value}))
        assert "INVALID_ARGUMENT" in str(e.value)
    room.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    room.gpu.render_hybrid(v, FRAME)
    for i in OWN:
        assert np.array_equal(before[i].view(np.uint8), room.gpu.read_hybrid(i).view(np.uint8)), i
    fresh = World(al.room_scene())
    with pytest.raises(rr.UtopianError, match="UH_HYBRID_AREA_LIGHTS without UH_HYBRID_DEFERRED"):
        fresh.gpu.render_hybrid(v, rr.HYBRID_GBUFFER | AREA)
    no_rt = room.view(raytracing_supported=0)
    with pytest.raises(rr.UtopianError, match="UH_HYBRID_AREA_LIGHTS casts shadow rays"):
        fresh.gpu.render_hybrid(no_rt, FRAME)
    with pytest.raises(rr.UtopianError, match="UH_HYBRID_AREA_LIGHTS casts its rays from the G-buffer"):
        fresh.gpu.render_hybrid(v, rr.HYBRID_DEFERRED | AREA)

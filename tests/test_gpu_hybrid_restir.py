"""GPU: the hybrid frame's reservoir lights (uh_render_hybrid's UH_HYBRID_RESTIR_LIGHTS) against the restatement of
tests/hybrid_restir_reference.py on the device's own G-buffer and reservoirs: the light-visibility image byte for byte with its ray counts,
the deferred output, known answers (no light, one light over a bare floor, the same light behind a box), edge shapes, the refusals,
isolation from the path tracer and stream order."""
import numpy as np
import pytest

import hybrid_restir_reference as rl
import rust_renderer_amd as rr
from hybrid_util import DEFERRED_ULP, bits, frame_view, gbuf, pair, read_all, synthetic_scene, ulps
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Mesh, Model, Scene, box, quad

pytestmark = pytest.mark.gpu

W, H = 67, 41
RESTIR = rr.HYBRID_RESTIR_LIGHTS
VIS = rr.HYBRID_LIGHT_VISIBILITY
# max |W_X - 1| over the reservoirs of the one-light scenes' three frames, measured with the oracle (whose reservoir passes the
# device's equal bit for bit): with one light every candidate is that light and W_X = (1 / p_hat) * W_sum / M is 1 up to rounding
ONE_LIGHT_WX_ERROR = 2.99e-7  # the bare floor: 2.98e-7 (5 ulp of 1); with the box: 2.38e-7


class World:
    """a scene on a GPU renderer and on the oracle with `lights` (GpuLight records) added to both, `frames` reservoir frames rendered on
    the GPU with the camera the hybrid views use"""

    def __init__(self, scene, lights, width=W, height=H, frames=3, mask=rr.PASS_RESTIR):
        self.scene, self.lights, self.size = scene, lights, (width, height)
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        for r in (self.gpu, self.cpu):
            for l in lights:
                r.add_gpu_light(l)
            r.initialize_raytracing()
        self.loop = rr.FrameLoop(self.gpu, scene.make_view(width, height))
        for _ in range(frames):
            self.loop.frame(mask)

    def view(self, num_lights=None, **kw):
        v = frame_view(self.scene, *self.size, **kw)
        v.num_lights = self.gpu.get_num_lights() if num_lights is None else num_lights
        return v

    def all_lights(self):
        """every light of the table in order: the scene's own (Scene.upload adds them first), then `lights`"""
        return [rr.make_light(p, (1.0, 1.0, 1.0), 1.0) for p in self.scene.lights] + list(self.lights)

    def check_visibility(self, v):
        """the device's visibility image and counts against the restatement on the device's G-buffer and reservoirs"""
        gpu = self.gpu
        g, res = gbuf(gpu), gpu.read_reservoirs(2)
        vis = gpu.read_hybrid(VIS)
        want, rays, occluded = rl.visibility(self.cpu, g, res, v, self.all_lights())
        s = gpu.hybrid_restir_stats()
        print(f"rays {s.rays} (restatement {rays}), occluded {s.occluded} (restatement {occluded}), differing texels {(vis != want).sum()}, pass {s.pass_ms:.3f} ms")
        assert np.array_equal(vis, want)
        assert (s.rays, s.occluded) == (rays, occluded)
        assert s.pass_ms > 0
        return g, res, vis, rl.cast_mask(g, res, v, self.all_lights())

    def check_deferred(self, v, g, res, vis, cast):
        """deferred_output against the restatement on the device's inputs: DEFERRED_ULP on the geometry pixels, bit for bit where no
        ray was cast"""
        gpu = self.gpu
        d = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        ref = rl.deferred(g, gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), v,
                          self.meshes, self.all_lights(), res, vis)
        geo = g["position"][..., 3] != 0
        assert geo.any() and np.isfinite(d[geo]).all()
        u = ulps(d[geo], ref[geo])
        quiet = geo & ~cast
        print(f"deferred: max {u.max()} ulp, exact on {(u == 0).mean():.4f} of the geometry pixels' channels; {quiet.sum()} geometry pixels cast no ray")
        assert u.max() <= DEFERRED_ULP
        assert np.array_equal(bits(d[quiet]), bits(ref[quiet]))
        assert gpu.hybrid_frame_stats().lights == 2
        return d


@pytest.fixture(scope="module")
def lit():
    """the synthetic scene with 8 point and spot lights behind its occluders, three reservoir frames with temporal and spatial reuse on"""
    return World(synthetic_scene(), rl.occluded_lights(8))


# ---- 1. visibility ------------------------------------------------------------------------------------------------------------
def test_visibility_equals_the_restatement_byte_for_byte(lit):
    v = lit.view()
    lit.gpu.render_hybrid(v, rr.HYBRID_GBUFFER | RESTIR)
    g, res, vis, cast = lit.check_visibility(v)
    assert set(np.unique(vis[cast])) == {0, 255}, "lit and occluded rays both occur"
    assert not vis[~cast].any()
    assert {int(l.light_type) for l in lit.lights} == {1, 2} and set(np.unique(res["Y"][cast])) <= set(range(8))


# ---- 2. the deferred output ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ssao, shadows", [(1, True), (0, True), (1, False), (0, False)])
def test_deferred_output_equals_the_restatement(lit, ssao, shadows):
    v = lit.view(ssao_enabled=ssao)
    mask = (rr.HYBRID_FRAME | RESTIR) & ~(0 if shadows else rr.HYBRID_RT_SHADOWS)
    if shadows:
        lit.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)  # rt_shadows reads the previous call's G-buffer: this camera's
    else:
        fresh = World(lit.scene, lit.lights)          # a context whose rt_shadows image is still its clear value
        lit = fresh
    lit.gpu.render_hybrid(v, mask)
    g, res, vis, cast = lit.check_visibility(v)
    sh = lit.gpu.read_hybrid(rr.HYBRID_SHADOWS)
    assert (sh == 255).all() != shadows
    d = lit.check_deferred(v, g, res, vis, cast)
    # the light is there: lit pixels are brighter than the same frame without any local light
    lit.gpu.render_hybrid(lit.view(0, ssao_enabled=ssao), rr.HYBRID_DEFERRED)
    dark = lit.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    typ = np.array([m["type"] for m in lit.meshes] + [0.0], np.float32)[np.minimum(g["pbr"][..., 3].astype(np.uint32), len(lit.meshes))]
    matte = (vis == 255) & (typ != 1.0)  # (a metal pixel shows its reflection alone)
    assert matte.any() and (d[matte][:, :3] >= dark[matte][:, :3]).all() and (d[matte][:, :3] > dark[matte][:, :3]).any()


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------
def test_no_lights_in_the_view_no_rays_and_the_plain_frame(lit):
    v = lit.view(0)
    lit.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)  # rt_shadows of both frames below reads this camera's G-buffer
    lit.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    plain = read_all(lit.gpu)
    lit.gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)
    s = lit.gpu.hybrid_restir_stats()
    assert (s.rays, s.occluded) == (0, 0) and s.pass_ms > 0 and not lit.gpu.read_hybrid(VIS).any()
    assert lit.gpu.hybrid_frame_stats().lights == 2
    with_bit = read_all(lit.gpu)
    for i in range(9):
        assert np.array_equal(plain[i].view(np.uint8), with_bit[i].view(np.uint8)), i


LIGHT = (0.4, 2.5, 0.3)


def floor_scene(with_box):
    """one point light over a floor (one cell, off-centre: no primary ray meets the shared edge); with_box: a box between the light and
    the part of the floor the camera sees in front of it"""
    fv, fi = quad((-23.0, 0.0, 19.0), (41.0, 0.0, 0.0), (0.0, 0.0, -43.0))
    meshes = [Mesh(fv, fi, rr.LAMBERTIAN, base_color=(0.8, 0.7, 0.6, 1.0))]
    if with_box:
        bv, bi = box((0.45, 1.2, 1.1), (1.3, 0.25, 0.9))
        meshes.append(Mesh(bv, bi, rr.LAMBERTIAN, base_color=(0.5, 0.6, 0.9, 1.0)))
    cam = rr.camera.Camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), 60.0, W / H, 0.01, 1000.0)
    return Scene("floor_box" if with_box else "floor", [(Model(meshes, []), None)], [LIGHT], cam)


def _within_the_one_light_bound(a, b):
    """|a - b| <= 4 ONE_LIGHT_WX_ERROR |b| + 4 ulp(b): W_X scales the light's term alone, which is at most the whole colour"""
    return (np.abs(a.astype(np.float64) - b) <= 4 * ONE_LIGHT_WX_ERROR * np.abs(b) + 4 * np.spacing(np.abs(b)).astype(np.float64)).all()


@pytest.mark.parametrize("with_box", [False, True])
def test_one_point_light_over_a_floor(with_box):
    w = World(floor_scene(with_box), [])
    gpu = w.gpu
    v = w.view()
    assert v.num_lights == 1
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)
    g, res, vis, cast = w.check_visibility(v)
    geo = g["position"][..., 3] != 0
    err = np.abs(res["W_X"][geo].astype(np.float64) - 1.0).max()
    print(f"max |W_X - 1| on the geometry pixels {err:.3e}")
    assert (res["Y"][geo] == 0).all() and err <= 4 * ONE_LIGHT_WX_ERROR
    d = w.check_deferred(v, g, res, vis, cast)
    gpu.render_hybrid(v, rr.HYBRID_DEFERRED)              # the plain one-light frame: unshadowed
    one = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    gpu.render_hybrid(w.view(0), rr.HYBRID_DEFERRED)      # and the frame without the light
    none = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    lit_px, hidden = vis == 255, cast & (vis == 0)
    print(f"geometry {geo.sum()}, lit {lit_px.sum()}, occluded {hidden.sum()}, facing away {(geo & ~cast).sum()}")
    assert _within_the_one_light_bound(d[lit_px], one[lit_px])
    assert (d[lit_px][:, :3] > none[lit_px][:, :3]).all()
    if not with_box:
        assert np.array_equal(lit_px, geo), "every floor pixel faces the light and sees it"
    else:
        assert lit_px.sum() >= 0.05 * geo.sum() and hidden.sum() >= 0.05 * geo.sum()
        assert np.array_equal(bits(d[hidden]), bits(none[hidden])), "an occluded pixel is the frame without the light"
        assert (one[hidden][:, :3] > none[hidden][:, :3]).all(), "which the plain deferred pass lights through the box"


# ---- 4. edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", [(5, 3), (64, 1), (129, 2)])
def test_small_and_odd_frames(width, height):
    """fewer pixels than a wave, one row of exactly a wave, and two rows that end inside a third block"""
    scene = synthetic_scene()
    if width > 8 * height:  # a strip: a narrow lens from the same place, or nearly every ray leaves the scene sideways
        scene.camera = rr.camera.Camera((0.0, 2.2, 6.5), (0.0, 0.5, 0.0), 1.2, width / height, 0.01, 1000.0)
    w = World(scene, rl.occluded_lights(8), width, height)
    v = w.view()
    w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    w.gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)
    g, res, vis, cast = w.check_visibility(v)
    assert cast.any()
    w.check_deferred(v, g, res, vis, cast)


def test_a_view_of_the_sky_alone_casts_nothing():
    scene = synthetic_scene()
    scene.camera = rr.camera.Camera((0.0, 2.2, 6.5), (0.0, 30.0, 5.0), 60.0, W / H, 0.01, 1000.0)
    w = World(scene, rl.occluded_lights(8))
    v = w.view()
    w.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)  # the trace kernel runs on an empty queue
    assert not (gbuf(w.gpu)["position"][..., 3] != 0).any()
    s = w.gpu.hybrid_restir_stats()
    assert (s.rays, s.occluded) == (0, 0) and s.pass_ms > 0 and not w.gpu.read_hybrid(VIS).any()
    assert np.array_equal(bits(w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), bits(plain))


def test_a_directional_light_and_an_empty_reservoir_cast_nothing():
    scene = synthetic_scene()
    lights = rl.occluded_lights(8)
    lights[2].light_type = 0.0
    w = World(scene, lights)
    gpu, v = w.gpu, w.view()
    gpu.render_hybrid(w.view(0), rr.HYBRID_GBUFFER | rr.HYBRID_DEFERRED)
    none = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    res = gpu.read_reservoirs(2)
    res["W_X"], res["W_sum"], res["M"] = 1.0, 1.0, 1
    res["Y"] = 2                      # the directional light everywhere ...
    res["Y"][::2, ::3] = -1           # ... or no light at all
    res["Y"][1::4, 1::5] = 5          # and a few pixels with a spot light
    gpu.write_reservoirs(2, res)
    gpu.render_hybrid(v, rr.HYBRID_DEFERRED | RESTIR)
    g, res2, vis, cast = w.check_visibility(v)
    assert np.array_equal(res2, res)
    assert cast.any() and not cast[res["Y"] != 5].any() and not vis[res["Y"] != 5].any()
    d = w.check_deferred(v, g, res, vis, cast)
    quiet = (g["position"][..., 3] != 0) & ~cast
    assert np.array_equal(bits(d[quiet]), bits(none[quiet])), "nothing added"


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(lit):
    gpu = lit.gpu
    v = lit.view()
    gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)
    before, vis_before, stats_before = read_all(gpu), gpu.read_hybrid(VIS), gpu.hybrid_restir_stats()

    def refused(view, mask, msg):
        with pytest.raises(UtopianError, match=msg) as e:
            gpu.render_hybrid(view, mask)
        assert "INVALID_ARGUMENT" in str(e.value)
        after = read_all(gpu)
        for i in range(9):
            assert np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8)), (msg, i)
        s = gpu.hybrid_restir_stats()
        assert np.array_equal(gpu.read_hybrid(VIS), vis_before) and (s.rays, s.occluded, s.pass_ms) == (stats_before.rays, stats_before.occluded, stats_before.pass_ms)

    other = synthetic_scene()
    other.camera = rr.camera.Camera((1.0, 1.5, 5.0), (0.0, 0.5, 0.0), 60.0, W / H, 0.01, 1000.0)
    moved = frame_view(other, W, H)  # another camera: a call that ran would change every image
    moved.num_lights = v.num_lights
    moved.raytracing_supported = 0
    refused(moved, rr.HYBRID_FRAME | RESTIR, "raytracing_supported")
    moved.raytracing_supported = 1
    moved.num_lights = v.num_lights + 1
    refused(moved, rr.HYBRID_FRAME | RESTIR, "num_lights exceeds")
    moved.num_lights = v.num_lights
    gpu.set_restir_partition(0, 2)
    try:
        refused(moved, rr.HYBRID_FRAME | RESTIR, "row partition")
    finally:
        gpu.set_restir_partition(0, 1)
    # a context without a G-buffer, and one without reservoirs
    no_gbuffer = World(lit.scene, lit.lights, frames=1)
    with pytest.raises(UtopianError, match="no G-buffer has been rendered"):
        no_gbuffer.gpu.render_hybrid(no_gbuffer.view(), RESTIR)
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
        no_gbuffer.gpu.read_hybrid(rr.HYBRID_POSITION)
    no_reservoirs = World(lit.scene, lit.lights, frames=0)
    no_reservoirs.gpu.render_hybrid(no_reservoirs.view(), rr.HYBRID_FRAME)
    with pytest.raises(UtopianError, match="no reservoir pass has run"):
        no_reservoirs.gpu.render_hybrid(no_reservoirs.view(), rr.HYBRID_FRAME | RESTIR)
    with pytest.raises(UtopianError, match="image 13"):
        no_reservoirs.gpu.read_hybrid(VIS)
    s = no_reservoirs.gpu.hybrid_restir_stats()
    assert (s.rays, s.occluded, s.pass_ms) == (0, 0, 0.0)
    no_reservoirs.loop.frame(rr.PASS_RESTIR)
    no_reservoirs.gpu.render_hybrid(no_reservoirs.view(), rr.HYBRID_FRAME | RESTIR)  # and with them it runs
    assert no_reservoirs.gpu.hybrid_restir_stats().rays > 0


# ---- 6. isolation and stream order --------------------------------------------------------------------------------------------
def _path_tracer_state(r):
    s = r.get_stats()
    out = dict(acc=bits(r.read_accumulation()), out=r.read_output_bgra8(), pos=bits(r.read_gbuffer_position()),
               stats=np.array(list(s.rays) + [s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses], np.uint64))
    for k in range(3):
        out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
    return out


def test_a_call_with_the_bit_changes_nothing_the_path_tracer_reads_and_later_calls_are_the_plain_ones():
    scene = synthetic_scene()
    a = World(scene, rl.occluded_lights(8), frames=3, mask=rr.PASS_ALL)
    b = World(scene, rl.occluded_lights(8), frames=3, mask=rr.PASS_ALL)
    v = a.view()
    before = _path_tracer_state(a.gpu)
    a.gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)
    after = _path_tracer_state(a.gpu)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert a.gpu.hybrid_restir_stats().rays > 0
    # the path tracer goes on as if the call had not been made
    a.loop.frame(rr.PASS_ALL)
    b.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    b.loop.frame(rr.PASS_ALL)
    sa, sb = _path_tracer_state(a.gpu), _path_tracer_state(b.gpu)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    # a later call without the bit equals the frame of a context that never set it
    a.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    b.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    ia, ib = read_all(a.gpu), read_all(b.gpu)
    for i in range(9):
        assert np.array_equal(ia[i].view(np.uint8), ib[i].view(np.uint8)), i


def test_frames_in_flight_then_the_hybrid_call_equal_the_serial_sequence():
    scene = synthetic_scene()

    def run(serial):
        w = World(scene, rl.occluded_lights(8), frames=0)
        v = w.view()
        w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        for _ in range(4):
            w.loop.frame(rr.PASS_ALL)
            if serial:
                w.gpu.synchronize()
        w.gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR)  # no wait in between
        w.loop.frame(rr.PASS_ALL)                           # and a frame behind it
        if serial:
            w.gpu.synchronize()
        s = w.gpu.hybrid_restir_stats()
        return dict(vis=w.gpu.read_hybrid(VIS), deferred=bits(w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), counts=np.array([s.rays, s.occluded]),
                    **_path_tracer_state(w.gpu))

    a, b = run(False), run(True)
    assert a["counts"][0] > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k

"""GPU: uh_denoise. Known answers on real frames (no restatement in the loop), the refusals, isolation from the path tracer and the hybrid
graph, the device against the restatement of tests/denoise_reference.py on the device's own read-backs, that it denoises, and stream order."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as dr
import rust_renderer_amd as rr
from hybrid_util import add_lights, bits, read_all, synthetic_scene
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Scene, quad

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(160, 120), (67, 45), (40, 24)]
# Colour and variance differ from the restatement only through the device's expf against numpy.exp: the largest relative difference
# (absolute floor 1e-6 of the image's maximum) measured over every case of test_device_equals_the_restatement on an MI355X, and the
# bound held, 4 x that (each side may be a couple of ulp off, and the error passes through up to five normalised sums). The worst
# value is the variance's: where a 7 x 7 neighbourhood is nearly uniform, m2 - m1 * m1 of the short-history estimate cancels down to a
# few ulp of m2, and a last-bit difference of a weight decides whether the clamp at 0 takes it ("Denoiser").
# The colour alone, which has no such cancellation, is held to its own, much smaller, measured value as well.
EXPF_MEASURED = 1.0
EXPF_HELD = 4 * EXPF_MEASURED
EXPF_COLOUR_MEASURED = 7.717e-05
EXPF_COLOUR_HELD = 4 * EXPF_COLOUR_MEASURED


class CornerScene(Scene):
    """two large perpendicular quads: an emissive white floor and a black wall"""

    def upload(self, renderer):
        white = renderer.default_diffuse_map()
        fv, fi = quad((-20.0, 0.0, 10.0), (40.0, 0.0, 0.0), (0.0, 0.0, -13.0), nu=4, nv=4)
        renderer.add_mesh(fv, fi, rr.make_material(rr.DIFFUSE_LIGHT, 0.0, (1.0, 1.0, 1.0, 1.0), diffuse_map=white))
        wv, wi = quad((-20.0, 0.0, -3.0), (40.0, 0.0, 0.0), (0.0, 30.0, 0.0), nu=4, nv=4)
        renderer.add_mesh(wv, wi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.0, 0.0, 0.0, 1.0), diffuse_map=white))
        renderer.initialize_raytracing()
        return renderer


def corner_scene():
    cam = rr.camera.Camera((0.0, 1.5, 4.0), (0.0, 1.0, -3.0), 60.0, 4.0 / 3.0, 0.01, 1000.0)
    return CornerScene("denoise_corner", [], [], cam, dict(sky_enabled=1))


SCENES = {"synthetic": synthetic_scene, "corner": corner_scene}


def projection_view(v):
    proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
    view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
    return tuple((proj @ view).astype(np.float32).T.reshape(-1))


class Rig:
    """a scene on a renderer; shoot() path-traces one frame of `spp` samples from the camera moved sideways by `shift` and casts the
    hybrid G-buffer with the same view; denoise() calls uh_denoise with the previous call's projection * view"""

    def __init__(self, name, size):
        self.scene, self.size = SCENES[name](), size
        self.gpu = rr.Renderer(*size)
        self.scene.upload(self.gpu)
        self.shots = 0
        self.prev_pv = None

    def view(self, shift=0.0):
        c = self.scene.camera
        cam = rr.camera.Camera(c.position + F([shift, 0, 0]), c.target + F([shift, 0, 0]), 60.0, self.size[0] / self.size[1], 0.01, 1000.0)
        v = rr.default_view(cam, *self.size)
        for k, val in self.scene.view_flags.items():
            setattr(v, k, val)
        v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
        v.use_ris_light_sampling = 0
        v.num_lights = self.gpu.get_num_lights()
        return v

    def shoot(self, v, spp=1, gbuffer=True):
        v.samples_per_frame = v.total_samples = spp
        v.time = 0.25 + 0.125 * self.shots  # another RNG stream per frame (frame number = total_samples + 10000 time)
        self.shots += 1
        self.gpu.render_frame(v, rr.PASS_REFERENCE_PT)
        if gbuffer:
            self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        return v

    def denoise(self, v, params):
        if self.prev_pv is not None:
            v.prev_frame_projection_view[:] = self.prev_pv
        self.gpu.denoise(v, params)
        self.prev_pv = projection_view(v)

    def reset(self):
        self.gpu.reset_denoise_history()
        self.prev_pv = None

    def inputs(self):
        g = self.gpu
        return (g.read_accumulation(), g.read_hybrid(rr.HYBRID_POSITION), g.read_hybrid(rr.HYBRID_NORMAL), g.read_hybrid(rr.HYBRID_ALBEDO),
                g.read_hybrid(rr.HYBRID_PBR))

    def images(self):
        g = self.gpu
        return dict(color=g.read_denoised(rr.DENOISE_COLOR), output=g.read_denoised(rr.DENOISE_OUTPUT), input=g.read_denoised(rr.DENOISE_INPUT),
                    temporal=g.read_denoised(rr.DENOISE_TEMPORAL_COLOR), history=g.read_denoised(rr.DENOISE_HISTORY),
                    variance=g.read_denoised(rr.DENOISE_VARIANCE))


_rigs = {}


def rig(name, size):
    """one renderer per scene and size for the whole module, its history cleared"""
    if (name, size) not in _rigs:
        _rigs[(name, size)] = Rig(name, size)
    r = _rigs[(name, size)]
    r.reset()
    r.shots = 0  # every test sees the same frames, whichever tests ran before it
    return r


def params(**kw):
    p = rr.default_denoise_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- 1. known answers on the device, no restatement in the loop ----------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_no_levels_no_flags_is_the_input_bit_for_bit(size):
    r = rig("synthetic", size)
    v = r.shoot(r.view(), spp=3)
    r.denoise(v, params(flags=0, iterations=0))
    im, acc = r.images(), r.gpu.read_accumulation()
    assert np.array_equal(bits(im["color"]), bits(im["input"]))
    assert np.array_equal(bits(im["input"][..., :3]), bits(acc[..., :3] / F(3.0))) and not im["color"][..., 3].any()
    assert np.array_equal(im["output"], r.gpu.read_output_bgra8()), "the path tracer's own sRGB conversion and packing"
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert geo.any() and not geo.all()
    assert np.array_equal(im["history"], geo.astype(np.float32))
    s = r.gpu.denoise_stats()
    assert s.geometry_pixels == geo.sum() and s.history_pixels == 0
    assert s.pass_ms[0] > 0 and s.pass_ms[1] > 0 and s.pass_ms[3] > 0


def test_camera_at_rest_accumulates_the_running_mean():
    r = rig("synthetic", (67, 45))
    k, p = 8, params(flags=rr.DENOISE_TEMPORAL, iterations=0, alpha_min=0.0)
    frames = []
    for _ in range(k):
        v = r.shoot(r.view())
        frames.append(r.gpu.read_accumulation()[..., :3])
        r.denoise(v, p)
    im = r.images()
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert not np.array_equal(frames[0], frames[1]), "each frame has its own samples"
    assert np.array_equal(im["history"], np.where(geo, F(k), F(0.0)))
    assert r.gpu.denoise_stats().history_pixels == geo.sum()
    stack = np.stack(frames).astype(np.float64)
    bound = 4 * k * 2.0 ** -23 * stack.max(axis=0)
    err = np.abs(im["temporal"][..., :3].astype(np.float64) - stack.mean(axis=0))
    print("running mean: largest error / bound", (err[geo] / np.maximum(bound[geo], 1e-300)).max())
    assert (err[geo] <= bound[geo]).all()
    assert np.array_equal(bits(im["temporal"][..., :3][~geo]), bits(frames[-1][~geo]))


def test_history_off_the_image_and_after_a_reset_is_one():
    r = rig("corner", (67, 45))
    p = params(iterations=1)
    geo = None
    for _ in range(2):
        v = r.shoot(r.view())
        r.denoise(v, p)
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert geo.sum() > 100 and (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 2).all()
    good = r.prev_pv
    off = np.array(good, np.float32).reshape(4, 4)  # [column][row]
    off[:, 0] += F(10.0) * off[:, 3]
    r.prev_pv = tuple(off.reshape(-1))
    r.denoise(r.shoot(r.view()), p)
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 1).all() and r.gpu.denoise_stats().history_pixels == 0
    r.denoise(r.shoot(r.view()), p)
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 2).all()
    r.gpu.reset_denoise_history()
    r.denoise(r.shoot(r.view()), p)
    h = r.gpu.read_denoised(rr.DENOISE_HISTORY)
    assert (h[geo] == 1).all() and not h[~geo].any() and r.gpu.denoise_stats().history_pixels == 0


@pytest.mark.parametrize("flags", [0, rr.DENOISE_TEMPORAL, rr.DENOISE_DEMODULATE, rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE])
def test_pixels_that_are_not_geometry_pass_through_bit_for_bit(flags):
    r = rig("synthetic", (67, 45))
    for shift in (0.0, 0.05):
        v = r.shoot(r.view(shift), spp=2)
        r.denoise(v, params(flags=flags))
        im, acc = r.images(), r.gpu.read_accumulation()
        sky = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] == 0
        assert sky.sum() > 50
        want = bits(acc[..., :3] / F(2.0))[sky]
        for name in ("color", "input", "temporal"):
            assert np.array_equal(bits(im[name][..., :3])[sky], want), name
        assert np.array_equal(im["output"][sky], r.gpu.read_output_bgra8()[sky])
        assert not im["history"][sky].any() and not im["variance"][sky].any()
        assert not np.array_equal(bits(im["color"][~sky]), bits(im["input"][~sky]))


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing_and_leave_the_history():
    fresh = Rig("corner", (40, 24))
    v = fresh.shoot(fresh.view(), gbuffer=False)
    with pytest.raises(UtopianError, match="reads the hybrid G-buffer"):
        fresh.gpu.denoise(v)
    with pytest.raises(UtopianError, match="before the first uh_denoise"):
        fresh.gpu.read_denoised(rr.DENOISE_COLOR)
    s = fresh.gpu.denoise_stats()
    assert (s.geometry_pixels, s.history_pixels, tuple(s.pass_ms)) == (0, 0, (0.0,) * 4)
    fresh.gpu.reset_denoise_history()  # allowed before the first call
    r = rig("corner", (40, 24))
    p = params(iterations=2)
    v = r.shoot(r.view())
    r.denoise(v, p)
    before = r.images()

    def refused(view, prm, match):
        with pytest.raises(UtopianError, match=match):
            r.gpu.denoise(view, prm)
        after = r.images()
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k

    r.gpu.set_tile_partition(0, 2, 16)
    try:
        refused(v, p, "tile partition")
    finally:
        r.gpu.set_tile_partition(0, 1, 16)
    zero = r.view()
    zero.total_samples = 0
    refused(zero, p, "is 0")
    refused(v, params(iterations=6), "iterations above 5")
    refused(v, params(flags=4), "unknown flag bits")
    refused(v, params(max_history=0), "max_history")
    refused(v, params(alpha_min=1.5), "alpha_min")
    refused(v, params(alpha_min=float("nan")), "alpha_min")
    refused(v, params(sigma_luminance=0.0), "sigma_luminance")
    refused(v, params(sigma_plane=float("inf")), "sigma_plane")
    refused(v, params(reproject_normal_cos=-1.5), "reproject_normal_cos")
    refused(v, params(reproject_plane=-1.0), "reproject_plane")
    bad = params()
    bad.reserved[2] = 1
    refused(v, bad, "reserved")
    with pytest.raises(ValueError, match="0..5"):
        r.gpu.read_denoised(6)
    fn = rr.api._bind(r.gpu._lib, "uh_", "read_denoised")
    assert fn(r.gpu._ctx, 6, before["color"].ctypes.data) == 1 and fn(r.gpu._ctx, -1, before["color"].ctypes.data) == 1
    # the history survived all of them: the next call of the camera at rest has history 2
    r.denoise(r.shoot(r.view()), p)
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 2).all()


# ---- 3. isolation -------------------------------------------------------------------------------------------------------------------
def _state(r):
    s = r.get_stats()
    out = dict(acc=bits(r.read_accumulation()), out=r.read_output_bgra8(), pos=bits(r.read_gbuffer_position()),
               stats=np.array(list(s.rays) + [s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses], np.uint64))
    for k in range(3):
        out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
    for i, img in read_all(r).items():
        out[f"hybrid{i}"] = img.view(np.uint8)
    return out


def test_a_call_changes_nothing_of_the_path_tracer_or_the_hybrid_graph():
    a, b = Rig("synthetic", (67, 45)), Rig("synthetic", (67, 45))
    views = []
    for r in (a, b):
        add_lights(r.gpu, 4, 7)
        v = r.view()
        v.use_ris_light_sampling = 1
        v.samples_per_frame = 1
        for _ in range(3):
            v.total_samples += 1
            r.gpu.render_frame(v, rr.PASS_ALL)
        r.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        r.gpu.render_hybrid(v, rr.HYBRID_FRAME)
        views.append(v)
    before = _state(a.gpu)
    for _ in range(2):
        a.denoise(rr.ViewUniformData.from_buffer_copy(views[0]), params())  # (a copy: denoise() writes prev_frame_projection_view)
    after = _state(a.gpu)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert a.gpu.denoise_stats().history_pixels > 0
    # and both go on alike
    for r, v in zip((a, b), views):
        v.total_samples += 1
        r.gpu.render_frame(v, rr.PASS_ALL)
        r.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    sa, sb = _state(a.gpu), _state(b.gpu)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


# ---- 4. the device against the restatement --------------------------------------------------------------------------------------
MOVE = 0.9  # sideways, per call: at these scenes' depths (2 to 7) 8 % of the frame's width or more, so a strip of the frame has no history


def rel_diff(got, want):
    floor = 1e-6 * float(np.abs(want).max())
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), max(floor, 1e-300))).max())


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("flags", [rr.DENOISE_TEMPORAL, rr.DENOISE_DEMODULATE, rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scene", ["synthetic", "corner"])
def test_device_equals_the_restatement(scene, size, flags, iterations):
    r = rig(scene, size)
    p = params(flags=flags, iterations=iterations)
    ref, pd = dr.Denoiser(), dr.params_of(p)
    worst = worst_colour = 0.0
    for call in range(4):
        v = r.shoot(r.view(MOVE * call))
        r.denoise(v, p)
        want, im = ref(*r.inputs(), v, pd), r.images()
        geo, kept = want["geometry"], want["kept"]
        s = r.gpu.denoise_stats()
        assert np.array_equal(bits(im["history"]), bits(want["history"])), "history length: bit for bit"
        assert (s.geometry_pixels, s.history_pixels) == (geo.sum(), kept.sum())
        assert np.array_equal(bits(im["input"]), bits(want["input"]))
        if call and (flags & rr.DENOISE_TEMPORAL):
            share = kept.sum() / geo.sum()
            print(f"call {call}: history kept on {share:.3f} of {geo.sum()} geometry pixels")
            assert 0.05 <= share <= 0.95, "kept and dropped histories both occur"
        else:
            assert not kept.any()
        # the temporal colour: the same float32 operations on the same inputs; held to the running mean's rounding
        acc_n = r.gpu.read_accumulation()[..., :3] / F(v.total_samples)
        scale = np.maximum(np.abs(want["temporal"][..., :3]), np.abs(acc_n)).astype(np.float64)
        assert (np.abs(im["temporal"][..., :3].astype(np.float64) - want["temporal"][..., :3]) <= 4 * (call + 1) * 2.0 ** -23 * scale).all()
        assert np.abs(im["output"].astype(int) - want["output"].astype(int)).max() <= 1, "the 8-bit image within 1 LSB"
        worst = max(worst, rel_diff(im["variance"], want["variance"]))
        worst_colour = max(worst_colour, rel_diff(im["color"][..., :3], want["color"][..., :3]))
    worst = max(worst, worst_colour)
    print(f"expf: largest relative difference of colour {worst_colour:.3e}, of colour and variance {worst:.3e}")
    assert worst <= EXPF_HELD and worst_colour <= EXPF_COLOUR_HELD


# ---- 5. it denoises ---------------------------------------------------------------------------------------------------------------
def test_it_denoises():
    r = rig("synthetic", (160, 120))
    step, calls = 0.02, 8
    final = r.view(step * (calls - 1))
    r.shoot(final, spp=2048, gbuffer=False)
    converged = r.gpu.read_accumulation()[..., :3].astype(np.float64) / 2048.0
    p = params()
    for call in range(calls):
        v = r.shoot(r.view(step * call))
        r.denoise(v, p)
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    mse = lambda img: float(((img[..., :3].astype(np.float64) - converged)[geo] ** 2).mean())
    noisy, temporal = mse(r.gpu.read_accumulation()), mse(r.gpu.read_denoised(rr.DENOISE_COLOR))
    r.reset()
    r.denoise(v, params(flags=rr.DENOISE_DEMODULATE))  # the same frame, spatial only
    spatial = mse(r.gpu.read_denoised(rr.DENOISE_COLOR))
    print(f"mse over geometry pixels: 1 spp {noisy:.5g}, spatial only {spatial:.5g} ({spatial / noisy:.4f} of it), "
          f"after {calls} calls {temporal:.5g} ({temporal / noisy:.4f})")
    assert spatial < noisy
    assert temporal < spatial


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------
def test_a_call_behind_four_frames_in_flight_equals_the_serial_sequence():
    def run(serial):
        r = Rig("synthetic", (67, 45))
        v = r.view()
        r.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        v.samples_per_frame = 1
        out = {}
        for rnd in range(2):
            for _ in range(4):
                v.total_samples += 1
                r.gpu.render_frame(v, rr.PASS_REFERENCE_PT)
                if serial:
                    r.gpu.synchronize()
            r.denoise(v, params())            # no wait in between
            v.total_samples += 1
            r.gpu.render_frame(v, rr.PASS_REFERENCE_PT)  # and a frame behind it, which adds to the accumulation the call reads
            if serial:
                r.gpu.synchronize()
            for k, img in r.images().items():
                out[f"{k}{rnd}"] = img.view(np.uint8)
        out["acc"] = bits(r.gpu.read_accumulation())
        return out

    a, b = run(False), run(True)
    assert a["history1"].view(np.float32).max() == 2
    for k in a:
        assert np.array_equal(a[k], b[k]), k

"""GPU: UH_HYBRID_TAA on the moving scene of motion_util.py under the sun-lit hybrid frame. That the bit changes nothing else, the device
against the restatement of tests/taa_reference.py on the device's own read-backs (bit for bit), the running mean of a camera at rest,
that a jittered sequence anti-aliases against a supersampled frame, that the clamp removes a moved panel's ghost, and the verbs and
refusals."""
import numpy as np
import pytest

import hybrid_frame_reference as fr
import rust_renderer_amd as rr
import taa_reference as tr
from hybrid_util import bits
from motion_util import ISO, PANEL, SIZES, WALL, MotionRig, mapped
from rust_renderer_amd.api import UtopianError
from test_gpu_denoise import projection_view

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = [pytest.param(False, id="cast"), pytest.param(True, id="raster")]
GBUFFER_AND_FRAME = (rr.HYBRID_POSITION, rr.HYBRID_NORMAL, rr.HYBRID_ALBEDO, rr.HYBRID_PBR, rr.HYBRID_SHADOWS, rr.HYBRID_REFLECTIONS,
                     rr.HYBRID_SSAO_IMAGE, rr.HYBRID_DEFERRED_OUTPUT)


class TaaRig(MotionRig):
    """the moving scene under HYBRID_FRAME: frame() renders one call - the view of the camera moved sideways by `shift`, jittered by
    taa_jitter(jitter) when that is not None, with the previous call's un-jittered projection * view - and returns the view it passed"""

    def frame(self, shift=0.0, jitter=None, taa=True, extra=0, time=None, **flags):
        v = self.view(shift)
        v.fxaa_enabled = 0
        for k, val in flags.items():
            setattr(v, k, val)
        if time is not None:
            v.time = time
        pv = projection_view(v)
        v.prev_frame_projection_view[:] = pv if self.prev_pv is None else self.prev_pv
        if jitter is not None:
            v = rr.Renderer.jitter_view(v, jitter, *self.size)
        self.gpu.render_hybrid(v, rr.HYBRID_FRAME | self.mask(True) | (rr.HYBRID_TAA if taa else 0) | extra)
        self.prev_pv = pv
        return v

    def read(self, *which):
        return [self.gpu.read_hybrid(w) for w in which]


# ---- 1. without the bit nothing moved ----------------------------------------------------------------------------------------------
def test_the_bit_changes_nothing_else_and_present_reads_its_output():
    plain, taa = TaaRig((67, 45)), TaaRig((67, 45))
    for step, shift in enumerate((0.0, 0.3, 0.6)):
        plain.frame(shift, taa=False)
        taa.frame(shift)
        for which in GBUFFER_AND_FRAME:
            a, b = plain.gpu.read_hybrid(which), taa.gpu.read_hybrid(which)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (step, which)
        sa, sb = plain.gpu.hybrid_frame_stats(), taa.gpu.hybrid_frame_stats()
        assert (sa.sky_pixels, sa.lights) == (sb.sky_pixels, sb.lights) and sa.sky_pixels > 0
        assert all((x > 0) == (y > 0) for x, y in zip(sa.pass_ms, sb.pass_ms)), "the same passes ran"
        d, out, p = taa.read(rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_TAA_OUTPUT, rr.HYBRID_PRESENT_OUTPUT)
        # present is exact given its source (hybrid_util.check_frame): taa_output on the rig with the bit, deferred_output on the other
        assert np.array_equal(p, fr.present(out, False)), step
        assert np.array_equal(plain.gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), fr.present(d, False)), step
        if step == 0:
            assert np.array_equal(bits(out), bits(d)), "no history yet: taa_output is deferred_output"
        else:
            assert not np.array_equal(bits(out), bits(d)) and not np.array_equal(p, fr.present(d, False)), "the history shows, and present shows it"
    assert plain.gpu.taa_stats().taa_ms == 0.0 and taa.gpu.taa_stats().taa_ms > 0.0


# ---- 2. the device equals the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raster", FORMS)
@pytest.mark.parametrize("size", SIZES)
def test_device_equals_the_restatement(size, raster):
    r, ref = TaaRig(size, raster), tr.Taa()
    W, H = size
    p = r.gpu.set_taa_params(flags=rr.TAA_CLAMP | rr.TAA_MOTION)

    def step(call, shift):
        v = r.frame(shift, jitter=call)
        d, pos, motion, out, n = r.read(rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_POSITION, rr.HYBRID_MOTION_IMAGE, rr.HYBRID_TAA_OUTPUT, rr.HYBRID_TAA_HISTORY)
        want = ref(d, pos, motion, v, tr.params_of(p), W, H)
        assert np.array_equal(bits(out), bits(want["output"])), call
        assert np.array_equal(bits(n), bits(want["history"])), call
        s = r.gpu.taa_stats()
        assert (s.history_pixels, s.reset_pixels) == (want["history_pixels"], want["reset_pixels"]) and s.history_pixels + s.reset_pixels == W * H
        return pos, n, want

    _, n, want = step(0, 0.0)
    assert (n == 1).all() and want["history_pixels"] == 0
    _, n, want = step(1, 0.3)  # the camera moves
    assert 0 < want["history_pixels"] < W * H, "a strip of the frame has no history"
    assert (n > 1.5).any()
    r.gpu.set_instance_transform(PANEL, rr.transform3x4((1.0, 1.0, 1.0), (0.5, 1.5, 0.2)))  # the panel moves rigidly
    step(2, 0.3)
    assert r.gpu.motion_stats().meshes_rigid == 1
    r.gpu.update_mesh_vertices(PANEL, mapped(r.panel_v, np.array([[1.05, 0, 0, 0.1], [0, 0.95, 0, -0.05], [0, 0, 1, 0.1]])))  # it deforms
    step(3, 0.3)
    assert r.gpu.motion_stats().meshes_deformed == 1
    r.gpu.update_isosurface_mesh(ISO, 3.0)  # the isosurface changes topology: no correspondence
    r.gpu.build_acceleration()
    pos, n, want = step(4, 0.3)
    iso = (pos[..., 3] != 0) & (r.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3] == ISO)
    assert iso.sum() >= 4 and (n[iso] == 1).all() and r.gpu.motion_stats().meshes_none == 1
    assert (n[~iso] > 1).any()


# ---- 3. the camera at rest: a running mean ------------------------------------------------------------------------------------------
def test_camera_at_rest_accumulates_the_running_mean():
    r = TaaRig((67, 45))
    r.gpu.set_taa_params(flags=0, alpha_min=0.0)
    r.gpu.set_rtao_params(samples=1, blur_radius=0)  # one occlusion ray per pixel, seeded by the frame number: the inputs differ per call
    inputs, x = [], None
    for k in range(5):
        r.frame(taa=True, extra=rr.HYBRID_RTAO, time=0.25 + 0.125 * k, ssao_enabled=1)
        d, out, n = r.read(rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_TAA_OUTPUT, rr.HYBRID_TAA_HISTORY)
        inputs.append(d)
        x = d[..., :3].copy() if x is None else x + (d[..., :3] - x) * (F(1.0) / F(k + 1))
        assert (n == k + 1).all(), k
        assert np.array_equal(bits(out[..., :3]), bits(x)), k
        assert np.array_equal(bits(out[..., 3]), bits(d[..., 3]))
    for a, b in zip(inputs, inputs[1:]):
        assert not np.array_equal(bits(a), bits(b)), "the ambient occlusion's noise differs from call to call"
    s = r.gpu.taa_stats()
    assert (s.history_pixels, s.reset_pixels) == (67 * 45, 0)


# ---- 4. it anti-aliases -----------------------------------------------------------------------------------------------------------
# The analytic slanted edge of test_taa_cpu.py gives 0.035 / 0.180 = 0.19 of the un-jittered error, and the bound there is one half. On
# the lit scene the ratio measured on an MI355X is 0.437 (307 edge pixels, 0.02043 against 0.04676): closer to one half than a factor of
# 1.5, so the measured ratio is what is held, with that factor of headroom ("Temporal anti-aliasing"). The lit
# frame's remaining error is not aliasing alone: the 4 x 4 truth also differs from any 67 x 45 frame in its screen-space ambient
# occlusion, which TAA does not touch.
TAA_RATIO_MEASURED = 0.437
TAA_RATIO_HELD = 1.5 * TAA_RATIO_MEASURED


def test_it_anti_aliases():
    W, H = 67, 45
    r, big = TaaRig((W, H)), TaaRig((4 * W, 4 * H))
    for rig in (r, big):  # twice: rt_shadows reads the previous call's G-buffer
        rig.frame(taa=False)
        rig.frame(taa=False)
    truth = big.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)[..., :3].astype(np.float64).reshape(H, 4, W, 4, 3).mean(axis=(1, 3))
    single = r.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)[..., :3].astype(np.float64)
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    mesh = np.where(geo, r.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3], -1.0)
    padded = np.pad(mesh, 1, mode="edge")
    around = np.stack([padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    edge = geo & (around != mesh[None]).any(axis=0)
    assert edge.sum() >= 40, edge.sum()
    for k in range(16):
        r.frame(jitter=k)
    out = r.gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT)[..., :3].astype(np.float64)
    e_taa, e_single = float(np.abs(out - truth)[edge].mean()), float(np.abs(single - truth)[edge].mean())
    print(f"taa: {edge.sum()} edge pixels, mean |taa_output - truth| {e_taa:.5f}, un-jittered single frame {e_single:.5f}, ratio {e_taa / e_single:.3f}")
    assert e_taa <= TAA_RATIO_HELD * e_single


# ---- 5. the clamp removes the ghost -------------------------------------------------------------------------------------------------
# The ghost test's lighting. Under the sun alone the wall is flat to float32: its 3 x 3 deviation (5e-6 to 4e-5 of a colour of 0.048,
# measured) is at the rounding floor of the contract's single-pass moments, sqrt(2^-22) * m1, so the device's box and a float64 box are
# different boxes there. A point light to the left in front gives the wall a gradient of about 1.5 % per pixel - twenty times that floor,
# a quarter of the 5 % of the colour difference the box may take - and lights the panel (albedo 0.7 to 0.9) several times brighter than
# the wall (0.3). No screen-space ambient occlusion: its pattern on the wall is not a gradient.
GHOST_LIGHT = dict(position=(-4.0, 1.4, 6.0), color=(10.0, 10.0, 10.0))


def _panel_steps(flags):
    """three calls, the panel 0.8 further to the side in each; returns the last call's input, output, position-derived masks"""
    r = TaaRig((67, 45))
    r.gpu.add_gpu_light(rr.make_light(**GHOST_LIGHT))
    r.gpu.initialize_raytracing()
    r.gpu.set_taa_params(flags=flags)
    was = None
    for k in range(3):
        r.gpu.set_instance_transform(PANEL, rr.transform3x4((1.0, 1.0, 1.0), (0.8 * k, 1.4, 0.0)))
        r.frame(ssao_enabled=0)
        pos, pbr = r.read(rr.HYBRID_POSITION, rr.HYBRID_PBR)
        before, was = was, (pos[..., 3] != 0) & (pbr[..., 3] == PANEL)
    wall = (pos[..., 3] != 0) & (pbr[..., 3] == WALL)
    d, out = r.read(rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_TAA_OUTPUT)
    return d[..., :3].astype(np.float64), out[..., :3].astype(np.float64), before, was, wall


def test_the_clamp_removes_the_ghost():
    c, out, before, panel, wall = _panel_steps(rr.TAA_CLAMP | rr.TAA_MOTION)
    H, W = wall.shape
    pad = np.pad(wall, 1, mode="constant")
    all_wall = np.all([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    Z = before & all_wall
    assert Z.sum() >= 8, Z.sum()
    cp = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")  # (Z's neighbourhoods lie inside the frame)
    nb = np.stack([cp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    m1, sg = nb.mean(axis=0), nb.std(axis=0)
    lo, hi = m1 - sg, m1 + sg  # clamp_gamma = 1
    delta = np.abs(c[panel].mean(axis=0) - c[Z].mean(axis=0))  # |panel colour - wall colour|, per channel
    width = (hi - lo)[Z].max(axis=0)
    print(f"taa ghost: {Z.sum()} pixels, colour difference {delta}, widest box {width}, largest excursion "
          f"{max(float((lo - out)[Z].max()), float((out - hi)[Z].max())):.3e}")
    assert (delta > 0).all() and (width < 0.05 * delta).all(), "the box is narrow against the ghost it has to remove"
    assert (out[Z] >= lo[Z] - 1e-6).all() and (out[Z] <= hi[Z] + 1e-6).all()
    # without the clamp the same pixels keep the panel
    c2, out2, before2, _, _ = _panel_steps(rr.TAA_MOTION)
    assert np.array_equal(before2, before) and np.array_equal(c2, c)
    assert (np.abs(out2 - c2)[Z] > 0.1 * delta).all()


# ---- 6. verbs and refusals ------------------------------------------------------------------------------------------------------------
def test_verbs_and_refusals():
    r = TaaRig((40, 24))
    g = r.gpu
    s = g.taa_stats()
    assert (s.history_pixels, s.reset_pixels, s.taa_ms, s.reserved) == (0, 0, 0.0, 0)
    v = r.view()
    v.fxaa_enabled = 0
    with pytest.raises(UtopianError, match="UH_HYBRID_TAA reprojects the G-buffer's positions, and no G-buffer has been rendered"):
        g.render_hybrid(v, rr.HYBRID_TAA | rr.HYBRID_DEFERRED)
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):  # nothing ran: not even the first-use allocation
        g.read_hybrid(rr.HYBRID_POSITION)
    # the motion flag over a G-buffer pass without the motion bit, in the call itself and left by an earlier one
    g.set_taa_params(flags=rr.TAA_CLAMP | rr.TAA_MOTION)
    with pytest.raises(UtopianError, match="the last G-buffer pass had no UH_HYBRID_MOTION"):
        g.render_hybrid(v, rr.HYBRID_FRAME | rr.HYBRID_TAA)
    g.render_hybrid(v, rr.HYBRID_FRAME)
    with pytest.raises(UtopianError, match="the last G-buffer pass had no UH_HYBRID_MOTION"):
        g.render_hybrid(v, rr.HYBRID_TAA)
    assert g.taa_stats().taa_ms == 0.0
    # the two images before the first pass: refused by the library, and by the Python layer before it asks
    buf = np.empty((24, 40, 4), np.float32)
    for which in (rr.HYBRID_TAA_OUTPUT, rr.HYBRID_TAA_HISTORY):
        assert g._api.read_hybrid(g._ctx, which, buf.ctypes.data) == 1
        assert b"images 16..17 before the first taa pass" in g._lib.uh_last_error(g._ctx)
        with pytest.raises(ValueError, match="once a render_hybrid call with HYBRID_TAA has run"):
            g.read_hybrid(which)
    assert g._api.read_hybrid(g._ctx, 18, buf.ctypes.data) == 1 and b"0..17" in g._lib.uh_last_error(g._ctx)
    # parameters out of range: refused with the reason, the old ones stay in force
    g.set_taa_params(flags=rr.TAA_CLAMP, max_history=2, alpha_min=0.0, clamp_gamma=1.5)
    for bad, why in ((dict(flags=4), "unknown flag bits"), (dict(flags=rr.TAA_CLAMP | 1 << 31), "unknown flag bits"), (dict(max_history=0), "max_history must be >= 1"),
                     (dict(alpha_min=-0.1), r"alpha_min must be in \[0, 1\]"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=float("nan")), "alpha_min"),
                     (dict(clamp_gamma=-1.0), "clamp_gamma must be finite and >= 0"), (dict(clamp_gamma=float("inf")), "clamp_gamma"),
                     (dict(clamp_gamma=float("nan")), "clamp_gamma")):
        with pytest.raises(UtopianError, match="uh_set_taa_params: " + why):
            g.set_taa_params(**bad)
    for k in range(3):
        r.frame()
    assert (g.read_hybrid(rr.HYBRID_TAA_HISTORY) == 2).all(), "max_history = 2 is still in force"
    s = g.taa_stats()
    assert s.taa_ms > 0 and (s.history_pixels, s.reset_pixels) == (40 * 24, 0)
    # a camera cut
    g.reset_taa_history()
    r.frame()
    assert (g.read_hybrid(rr.HYBRID_TAA_HISTORY) == 1).all()
    s = g.taa_stats()
    assert (s.history_pixels, s.reset_pixels) == (0, 40 * 24)
    assert np.array_equal(bits(g.read_hybrid(rr.HYBRID_TAA_OUTPUT)), bits(g.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)))
    # a refused call leaves the history: the next pass has N = 2
    g.set_taa_params(flags=rr.TAA_MOTION, max_history=2, alpha_min=0.0, clamp_gamma=1.5)
    g.render_hybrid(v, rr.HYBRID_GBUFFER)
    with pytest.raises(UtopianError, match="had no UH_HYBRID_MOTION"):
        g.render_hybrid(v, rr.HYBRID_TAA)
    g.set_taa_params(flags=rr.TAA_CLAMP, max_history=2, alpha_min=0.0, clamp_gamma=1.5)
    r.frame()
    assert (g.read_hybrid(rr.HYBRID_TAA_HISTORY) == 2).all()
    # a later call without the bit leaves taa_output as it was, and present reads deferred_output again
    kept, kept_n = g.read_hybrid(rr.HYBRID_TAA_OUTPUT), g.read_hybrid(rr.HYBRID_TAA_HISTORY)
    r.frame(0.4, taa=False)
    assert np.array_equal(bits(g.read_hybrid(rr.HYBRID_TAA_OUTPUT)), bits(kept)) and np.array_equal(g.read_hybrid(rr.HYBRID_TAA_HISTORY), kept_n)
    d = g.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    assert not np.array_equal(bits(d), bits(kept))
    assert np.array_equal(g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), fr.present(d, False))

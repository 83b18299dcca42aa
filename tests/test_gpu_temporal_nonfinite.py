"""GPU: the rule of uh_denoise and UH_HYBRID_TAA for samples that are not finite ("Non-finite input"): a bad pixel
passes through and takes part in nothing. No verb writes the accumulation or deferred_output, so the bad samples come from the scene of
motion_util.py. An emitter's colour is not the way: the path tracer's emitters emit (1, 1, 1) whatever their base colour (rchit:85-89).
A Lambertian surface's base colour multiplies the path's throughput, and nothing refuses it: small squares of base colour 3e38 just
before a surface - the light their paths find next, the floor's 1 or the sky's, comes back times 3e38, finite with an overflowing
square, and two such samples accumulate to +Inf -, of +Inf itself, of 1e30 (finite, its square is not) and of (NaN, 1, 1); and spot lights of colour 2e38 close to a surface, whose
deferred sum overflows in their cones. The squares and the cones are aimed at the centres of floor or wall pixels read from a scouting
G-buffer: small ones inside one pixel, so that B has pixels all of whose neighbours are good, and large ones over a 2 x 2 block, so
that the next call has pixels whose history taps all fall on B. Three calls each - clean,
bad, clean, the camera 0.3 further to the side in each - with the squares under the floor and the lights switched off in the clean ones.
Every call is held to the restatements (denoise_reference.py, denoise_motion_reference.py, taa_reference.py) as test_gpu_denoise.py and
test_gpu_taa.py hold them, and the properties of test_denoise_cpu.py / test_taa_cpu.py are asserted on the device's own images.
deferred_output holds no NaN in this scene (a NaN light colour would be NaN * 0 in every pixel outside its cone, the whole frame); the
CPU tests cover it."""
import numpy as np
import pytest

import denoise_motion_reference as dmr
import denoise_reference as dr
import hybrid_frame_reference as fr
import rust_renderer_amd as rr
import taa_reference as tr
import temporal_cases as tc
from hybrid_util import bits
from motion_util import FLOOR, PANEL, SIZES, WALL, MotionRig
from rust_renderer_amd.scenes import quad
from temporal_gpu_util import TemporalRig, hold_denoise, hold_expf, hold_taa, isolated, quiet_pixels
from test_gpu_denoise import params

pytestmark = pytest.mark.gpu

F = np.float32
SHIFT = 0.3
HOT, INF_MESH, LARGE, NAN_MESH = 4, 5, 6, 7
SHOWN, HIDDEN = rr.transform3x4(), rr.transform3x4((1.0, 1.0, 1.0), (0.0, -1000.0, 0.0))


def panel_at(call):
    return rr.transform3x4((1.0, 1.0, 1.0), (0.0, 1.4, 0.1 * call))


class Scout:
    """the pixels to aim at, from the G-buffer of the bad call's view: `picks` [(x, y)] on the floor and the wall, each in a 5 x 5
    neighbourhood of its own mesh, with their world points, normals and the width of a pixel at their depth"""

    def __init__(self, size, count):
        s = MotionRig(size)
        v = s.view(SHIFT)
        pos, mesh, geo, _ = s.gbuffer(v, motion=False)
        self.pos = pos
        self.normal = s.gpu.read_hybrid(rr.HYBRID_NORMAL)
        self.picks = quiet_pixels(pos, mesh, (FLOOR, WALL), count)
        iv = np.array(v.inverse_view[:], np.float64).reshape(4, 4).T  # columns: right, up, back, eye
        self.right, self.up, self.back, self.eye = iv[:3, 0], iv[:3, 1], iv[:3, 2], iv[:3, 3]
        self.rows = size[1]

    def point(self, x, y):
        return self.pos[y, x, :3].astype(np.float64)

    def pixel(self, p):
        """the width of a pixel at the depth of world point p (60 degrees of height)"""
        return float(np.dot(self.eye - p, self.back)) * 2.0 * np.tan(np.radians(30.0)) / self.rows

    def billboard(self, p, pixels):
        """a square facing the camera, `pixels` pixels wide on screen, centred on the ray to p, two hundredths of a unit before it"""
        c = p + (self.eye - p) / np.linalg.norm(self.eye - p) * 0.02
        side = pixels * self.pixel(p)
        return quad(c - (self.right + self.up) * side / 2, self.right * side, self.up * side)


def merged(parts):
    vs, idx, base = [], [], 0
    for v, i in parts:
        vs.append(v)
        idx.append(np.asarray(i, np.uint32).reshape(-1) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(idx)


SMALL = 0.99  # of a pixel: a sample of the pixel meets the square (all but 2 % of the pixel's area), a sample of its neighbours cannot


class FireflyRig(MotionRig):
    """motion_util's scene with the Lambertian squares whose base colour no radiance survives: of 3e38 one over a 2 x 2 block (around
    the corner where its four pixels meet), one inside a pixel each of +Inf and of 1e30, and two of (NaN, 1, 1)"""

    def __init__(self, size):
        super().__init__(size)
        sc = Scout(size, 5)
        g = self.gpu
        white = g.default_diffuse_map()
        lambert = lambda *rgb: rr.make_material(rr.LAMBERTIAN, 0.0, rgb + (1.0,), diffuse_map=white)
        x, y = sc.picks[2]
        corner = (sc.point(x, y) + sc.point(x + 1, y + 1)) / 2
        hv, hi = sc.billboard(corner, 2.6)
        assert g.add_mesh(hv, hi, lambert(3e38, 3e38, 3e38), HIDDEN) == HOT
        iv, ii = sc.billboard(sc.point(*sc.picks[0]), SMALL)
        assert g.add_mesh(iv, ii, lambert(float("inf"), float("inf"), float("inf")), HIDDEN) == INF_MESH
        lv, li = sc.billboard(sc.point(*sc.picks[1]), SMALL)
        assert g.add_mesh(lv, li, lambert(1e30, 1e30, 1e30), HIDDEN) == LARGE
        nv, ni = merged([sc.billboard(sc.point(*sc.picks[3]), SMALL), sc.billboard(sc.point(*sc.picks[4]), SMALL)])
        assert g.add_mesh(nv, ni, lambert(float("nan"), 1.0, 1.0), HIDDEN) == NAN_MESH
        g.initialize_raytracing()

    def show(self, shown):
        for m in (HOT, INF_MESH, LARGE, NAN_MESH):
            self.gpu.set_instance_transform(m, SHOWN if shown else HIDDEN)


def kinds_after(taps, bad_before, history):
    """the call after B: a pixel whose taps all fall on B starts again, and some pixel with taps on and off B keeps a history"""
    only_bad, mixed, clean = tc.tap_kinds(taps, bad_before)
    assert only_bad.any() and mixed.any() and clean.any(), "all three kinds of pixel exist"
    assert (history[only_bad] <= 1).all(), "nothing to fetch: the history starts again"
    assert (history[mixed] > 1).any(), "renormalised over the taps that remain"


DENOISE_CASES = [pytest.param(rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE, 2, id="2spp"), pytest.param(rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE, 1, id="1spp"),
                 pytest.param(rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE | rr.DENOISE_MOTION, 2, id="motion-2spp")]


@pytest.mark.parametrize("flags,spp", DENOISE_CASES)
@pytest.mark.parametrize("size", SIZES)
def test_the_denoiser_contains_fireflies(size, flags, spp):
    r = FireflyRig(size)
    motion = bool(flags & rr.DENOISE_MOTION)
    p = params(flags=flags)
    ref, params_of = (dmr.MotionDenoiser(), dmr.params_of) if motion else (dr.Denoiser(), dr.params_of)
    worst = worst_colour = 0.0
    before = None
    for call in range(3):
        r.show(call == 1)
        if motion:
            r.gpu.set_instance_transform(PANEL, panel_at(call))  # the panel approaches: its history follows the motion image
        v = r.shoot(r.view(SHIFT * call), spp=spp)
        r.denoise(v, p)
        inputs = r.inputs()
        want, im, a, b = hold_denoise(r, ref, inputs if motion else inputs[:5], v, p, params_of, call)
        worst, worst_colour = max(worst, a), max(worst_colour, b)
        B, drawn = want["bad"], want["geometry"]
        raw = inputs[0][..., :3] / F(spp)
        floats = ("color", "input", "temporal", "history", "variance")
        if call != 1:
            assert not B.any(), "a clean call"
            for name in floats:
                assert np.isfinite(im[name]).all(), (call, name)
            if call == 2:
                kinds_after(ref.taps, before, im["history"])
                if motion:
                    on_panel = drawn & (inputs[4][..., 3] == PANEL)
                    assert on_panel.any() and (im["history"][on_panel] > 1).mean() >= 0.5, "the moving panel keeps its history"
            continue
        before = B
        nan, inf, big = np.isnan(raw).any(axis=-1), np.isinf(raw).any(axis=-1) & ~np.isnan(raw).any(axis=-1), np.isfinite(raw).all(axis=-1)
        print(f"B: {B.sum()} of {drawn.sum()} geometry pixels, {isolated(B).sum()} isolated; NaN {(B & nan).sum()}, Inf {(B & inf).sum()}, "
              f"finite with an overflowing square {(B & big).sum()}")
        assert B.any() and 10 * B.sum() <= drawn.sum() and isolated(B).any()
        assert (B & nan).any(), "the square whose red is NaN"
        assert (B & inf).any(), "the square of +Inf; at two samples also 3e38 times the floor's 1, twice"
        assert (B & big).any(), "1e30 times a radiance: finite, and its square is not"
        assert np.array_equal(B, drawn & ~dr.sample_ok(raw)), "B, from the device's read-back of its input"
        for name in ("color", "input", "temporal"):
            assert np.array_equal(bits(im[name][..., :3])[B], bits(raw)[B]), name
        assert not im["history"][B].any() and not want["kept"][B].any()
        for name in floats:
            assert np.isfinite(im[name][~B]).all(), name
        s = r.gpu.denoise_stats()
        assert s.geometry_pixels == drawn.sum() and s.history_pixels == (im["history"] > 1).sum()
    hold_expf(worst, worst_colour)


def spot(aim, normal, distance, exponent, colour):
    """a spot light `distance` above the surface point `aim` along its normal, shining back along it"""
    l = rr.make_light(tuple(aim + normal * distance), color=(colour,) * 3)
    l.light_type = 2.0
    l.direction[:] = [float(a) for a in normal]  # from the surface towards the light
    l.spot = exponent
    return l


@pytest.mark.parametrize("flags", [pytest.param(rr.TAA_CLAMP, id="clamp"), pytest.param(0, id="free"), pytest.param(rr.TAA_CLAMP | rr.TAA_MOTION, id="clamp-motion")])
@pytest.mark.parametrize("size", SIZES)
def test_taa_contains_an_overflowing_deferred_sum(size, flags):
    r = TemporalRig(size)
    sc = Scout(size, 2)
    aim = [(sc.point(x, y), sc.normal[y, x, :3].astype(np.float64)) for x, y in sc.picks]
    # two lights of 2e38 one unit above a pixel's point: 10 / d^2 of it each in the cone's axis, +Inf; cos^360 leaves the 2^48 of the
    # rule 0.6 units from the axis. One of 3e38 above another pixel's point, cos^4000, so near that 2^48 is left a third of a pixel
    # from the axis
    near = 0.3 * sc.pixel(aim[1][0]) / 0.17  # cos^4000 of atan(0.17) is 1e-25
    for l in (spot(*aim[0], 1.0, 360.0, 2e38), spot(*aim[0], 1.0, 360.0, 2e38), spot(*aim[1], near, 4000.0, 3e38)):
        r.gpu.add_gpu_light(l)
    r.gpu.initialize_raytracing()
    p = r.gpu.set_taa_params(flags=flags)
    ref = tr.Taa()
    before = None
    for call in range(3):
        if flags & rr.TAA_MOTION:
            r.gpu.set_instance_transform(PANEL, panel_at(call))
        v = r.step(SHIFT * call, None, num_lights=3 if call == 1 else 0)
        want, d, out, n = hold_taa(r, ref, v, p)
        B = want["bad"]
        geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
        present = r.gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
        # present's texture() fetch at a texel's centre still multiplies the texels to its right and below by a weight of 0: it is held
        # where none of those four is in B
        pad = np.pad(B, ((0, 1), (0, 1)), mode="edge")
        reach = pad[:-1, :-1] | pad[:-1, 1:] | pad[1:, :-1] | pad[1:, 1:]
        with np.errstate(all="ignore"):
            assert np.array_equal(present[~reach], fr.present(out, False)[~reach]), "present reads taa_output"
        if call != 1:
            assert not B.any() and np.isfinite(out).all() and (n >= 1).all(), "a clean call"
            if call == 2:
                kinds_after(ref.taps, before, n)
            continue
        before = B
        c = d[..., :3]
        inf, big = np.isinf(c).any(axis=-1), np.isfinite(c).all(axis=-1)
        print(f"B: {B.sum()} of {geo.sum()} geometry pixels, {isolated(B).sum()} isolated; NaN {np.isnan(c).any(axis=-1).sum()}, Inf {(B & inf).sum()}, "
              f"finite and above 2^48 {(B & big).sum()}")
        assert B.any() and 10 * B.sum() <= geo.sum() and isolated(B).any()
        assert (B & inf).any() and (B & big).any()
        assert np.array_equal(B, ~tr.sample_ok(c)), "B, from the device's read-back of its input"
        assert np.array_equal(bits(out)[B], bits(d)[B]), "the input, bits unchanged"
        assert not n[B].any() and (n[~B] >= 1).all() and np.isfinite(out[~B]).all()
        assert not want["blended"][B].any(), "B counts in reset_pixels"
        s = r.gpu.taa_stats()
        assert s.history_pixels + s.reset_pixels == size[0] * size[1] and s.history_pixels == (n > 1).sum()

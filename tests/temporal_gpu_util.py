"""Shared by test_gpu_temporal_sizes.py and test_gpu_temporal_nonfinite.py: the moving scene of motion_util.py with both temporal filters
running in every call - a path-traced frame, the hybrid frame with UH_HYBRID_MOTION and UH_HYBRID_TAA, then uh_denoise - and the
comparisons of test_gpu_denoise.py, test_gpu_denoise_motion.py and test_gpu_taa.py against the restatements, with their tolerances.
Not a test module."""
import numpy as np

import rust_renderer_amd as rr
import taa_reference as tr
from hybrid_util import bits
from motion_util import MotionRig
from test_gpu_denoise import EXPF_COLOUR_HELD, EXPF_HELD, projection_view, rel_diff

F = np.float32


class TemporalRig(MotionRig):
    """step() is one call of everything: the view of the camera moved sideways by `shift` with the previous call's projection * view"""

    def __init__(self, size, raster=False, eye_target=None, fov=60.0):
        super().__init__(size, raster)
        self.fov = fov
        if eye_target is not None:
            self.scene.camera = rr.camera.Camera(eye_target[0], eye_target[1], fov, size[0] / size[1], 0.01, 1000.0)

    def view(self, shift=0.0):
        """Rig.view with this rig's vertical field of view"""
        c = self.scene.camera
        cam = rr.camera.Camera(c.position + F([shift, 0, 0]), c.target + F([shift, 0, 0]), self.fov, self.size[0] / self.size[1], 0.01, 1000.0)
        v = rr.default_view(cam, *self.size)
        for k, val in self.scene.view_flags.items():
            setattr(v, k, val)
        v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
        v.use_ris_light_sampling = 0
        v.num_lights = self.gpu.get_num_lights()
        v.rebuild_tlas = 1
        return v

    def step(self, shift, denoise_params, spp=1, taa=True, num_lights=None):
        g = self.gpu
        v = self.view(shift)
        v.fxaa_enabled = 0
        if num_lights is not None:
            v.num_lights = num_lights
        v.samples_per_frame = v.total_samples = spp
        v.time = 0.25 + 0.125 * self.shots
        self.shots += 1
        pv = projection_view(v)
        v.prev_frame_projection_view[:] = pv if self.prev_pv is None else self.prev_pv
        g.render_frame(v, rr.PASS_REFERENCE_PT)
        g.render_hybrid(v, rr.HYBRID_FRAME | self.mask(True) | (rr.HYBRID_TAA if taa else 0))
        if denoise_params is not None:
            g.denoise(v, denoise_params)
        self.prev_pv = pv
        return v


def hold_denoise(r, ref, inputs, v, p, params_of, call):
    """the device's uh_denoise images against the restatement `ref` on the device's own inputs: history, input and the stats bit for
    bit, the temporal colour to the running mean's rounding, the 8-bit image within 1 LSB; returns (want, images, the largest relative
    difference of the variance, of the colour) - the caller holds those two to EXPF_HELD and EXPF_COLOUR_HELD over its calls. A bad
    pixel's colour passes through and may not be finite: there the bits are held"""
    want, im = ref(*inputs, v, params_of(p)), r.images()
    geo, kept, bad = want["geometry"], want["kept"], want["bad"]
    s = r.gpu.denoise_stats()
    assert np.array_equal(bits(im["history"]), bits(want["history"])), "history length: bit for bit"
    assert (s.geometry_pixels, s.history_pixels) == (geo.sum(), kept.sum())
    assert np.array_equal(bits(im["input"]), bits(want["input"]))
    for name in ("temporal", "color"):
        assert np.array_equal(bits(im[name])[bad], bits(want[name])[bad]), name
    ok = ~bad
    acc_n = inputs[0][..., :3] / F(v.total_samples)
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(want["temporal"][..., :3]), np.abs(acc_n)).astype(np.float64)
        near = np.abs(im["temporal"][..., :3].astype(np.float64) - want["temporal"][..., :3]) <= 4 * (call + 1) * 2.0 ** -23 * scale
    same = bits(im["temporal"][..., :3]) == bits(want["temporal"][..., :3])  # (a sky pixel that is not finite passes through as well)
    assert (near | same)[ok].all()
    assert np.abs(im["output"].astype(int) - want["output"].astype(int))[ok].max(initial=0) <= 1, "the 8-bit image within 1 LSB"
    finite = ok & np.isfinite(want["color"]).all(axis=-1)
    assert np.array_equal(bits(im["color"])[ok & ~finite], bits(want["color"])[ok & ~finite])
    worst = rel_diff(im["variance"], want["variance"])
    worst_colour = rel_diff(im["color"][..., :3][finite], want["color"][..., :3][finite]) if finite.any() else 0.0
    return want, im, worst, worst_colour


def hold_expf(worst, worst_colour):
    worst = max(worst, worst_colour)
    print(f"expf: largest relative difference of colour {worst_colour:.3e}, of colour and variance {worst:.3e}")
    assert worst <= EXPF_HELD and worst_colour <= EXPF_COLOUR_HELD


def hold_taa(r, ref, v, p):
    """the device's taa_output and history length against the restatement on the device's own read-backs, bit for bit, and the stats;
    returns (want, deferred_output, taa_output, history length)"""
    W, H = r.size
    g = r.gpu
    d, pos, motion = g.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), g.read_hybrid(rr.HYBRID_POSITION), g.read_hybrid(rr.HYBRID_MOTION_IMAGE)
    out, n = g.read_hybrid(rr.HYBRID_TAA_OUTPUT), g.read_hybrid(rr.HYBRID_TAA_HISTORY)
    want = ref(d, pos, motion, v, tr.params_of(p), W, H)
    assert np.array_equal(bits(out), bits(want["output"]))
    assert np.array_equal(bits(n), bits(want["history"]))
    s = g.taa_stats()
    assert (s.history_pixels, s.reset_pixels) == (want["history_pixels"], want["reset_pixels"]) and s.history_pixels + s.reset_pixels == W * H
    return want, d, out, n


def isolated(bad):
    """the pixels of `bad` (H, W) whose eight neighbours all lie in the frame and outside `bad`"""
    H, W = bad.shape
    pad = np.pad(bad, 1, mode="constant", constant_values=True)  # outside the frame counts against a pixel
    around = np.sum([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
    return bad & (around == 0)


def quiet_pixels(pos, mesh, meshes, count, margin=2, apart=5):
    """`count` pixels (x, y) of a G-buffer whose (2 margin + 1)^2 neighbourhood lies in the frame and on one of `meshes` (the same one),
    at least `apart` pixels from one another, in scan order"""
    H, W = mesh.shape
    geo = pos[..., 3] != 0
    found = []
    for y in range(margin, H - margin):
        for x in range(margin, W - margin):
            around = (slice(y - margin, y + margin + 1), slice(x - margin, x + margin + 1))
            if mesh[y, x] in meshes and geo[around].all() and (mesh[around] == mesh[y, x]).all() and all(max(abs(x - a), abs(y - b)) >= apart for a, b in found):
                found.append((x, y))
                if len(found) == count:
                    return found
    raise AssertionError(f"only {len(found)} of {count} quiet pixels")

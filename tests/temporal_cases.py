"""Shared by the tests of the temporal filters' rule for non-finite input (test_denoise_cpu.py, test_taa_cpu.py): a wall facing a camera
that moves sideways from call to call, the set B of bad pixels those tests plant in one call, and the finite sequences whose outputs
tests/golden/temporal_finite.npz keeps from the restatements as they were before the rule. Not a test module."""
import numpy as np

import rust_renderer_amd as rr
import taa_reference as tr

F = np.float32
W, H = 97, 61
CALLS, STEP = 6, 0.07  # 0.07 is about half a pixel at the wall's depth: two history taps per pixel, one texel apart
OVERFLOWING = F(2e19)  # finite, and its luminance squared is not

# (x, y, channel, value): a 2 x 2 block in the interior - the pixel whose taps are that block keeps nothing - with one value of each
# kind, a pixel on each of two frame edges and two corners
B = [(48, 30, 0, F(np.inf)), (49, 30, 1, F(-np.inf)), (48, 31, 2, F(np.nan)), (49, 31, None, OVERFLOWING),
     (0, 20, 2, F(np.inf)), (30, 0, 0, F(np.nan)), (W - 1, H - 1, None, OVERFLOWING), (0, 0, 1, F(-np.inf)), (W - 1, 0, 0, F(np.nan))]


def projection_view(v):
    proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
    view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
    return tuple((proj @ view).astype(np.float32).T.reshape(-1))


def b_mask(w=W, h=H):
    m = np.zeros((h, w), bool)
    for x, y, _, _ in B:
        m[y, x] = True
    return m


def plant(image, scale=1.0):
    """a copy of an (H, W, 4) image with B's values (times `scale`: the accumulation of n samples holds n times the colour) in place"""
    out = image.copy()
    for x, y, ch, val in B:
        out[y, x, slice(0, 3) if ch is None else ch] = val * F(scale)
    return out


def wall_call(k, w=W, h=H, step=STEP, samples=1):
    """call k of the sequence: the camera at (k step, 1.5, 4) looks down -z at the wall z = -3, which fills the frame; the view carries
    the previous call's projection * view (its own in call 0). Returns dict(view, position, normal, albedo, pbr, motion): motion is the
    position with w = 1 (nothing moves but the camera)"""
    eye = lambda i: rr.camera.Camera((step * i, 1.5, 4.0), (step * i, 1.5, -3.0), 60.0, w / h, 0.01, 1000.0)
    v = rr.default_view(eye(k), w, h)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    v.total_samples, v.accumulation_limit = samples, 999999
    v.prev_frame_projection_view[:] = projection_view(rr.default_view(eye(max(k - 1, 0)), w, h))
    d = tr.primary_directions(v, w, h).astype(np.float64)
    o = np.array(v.inverse_view[12:15], np.float64)
    t = (-3.0 - o[2]) / d[:, 2]
    pos = np.ones((h, w, 4), np.float32)
    pos[..., :3] = (o + t[:, None] * d).astype(np.float32).reshape(h, w, 3)
    nrm = np.tile(np.array([0, 0, 1, 1], np.float32), (h, w, 1))
    alb = np.random.default_rng(77).integers(0, 256, (h, w, 4), dtype=np.uint8)  # the wall's own pattern: the same in every call
    alb[h // 2, w // 2 + 3, :3] = 0  # the 0.01 floor of the demodulator
    return dict(view=v, position=pos, normal=nrm, albedo=alb, pbr=np.zeros((h, w, 4), np.float32), motion=pos.copy())


def wall_noise(k, w=W, h=H, lo=0.5, hi=0.6):
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = np.random.default_rng(100 + k).uniform(lo, hi, (h, w, 3)).astype(np.float32)
    return a


def tap_kinds(taps, bad):
    """from a restatement's `taps` of a call - (in the frame with a weight, index, weight) for each of the four - and the (H, W) mask of
    the PREVIOUS call's bad pixels: which pixels have all their taps on bad texels, which have some on and some off, and which have
    taps and none on a bad texel; three (H, W) masks"""
    flat = bad.reshape(-1)
    on = sum((valid & flat[j]).astype(int) for valid, j, _ in taps)
    off = sum((valid & ~flat[j]).astype(int) for valid, j, _ in taps)
    return ((on > 0) & (off == 0)).reshape(bad.shape), ((on > 0) & (off > 0)).reshape(bad.shape), ((on == 0) & (off > 0)).reshape(bad.shape)


def renormalised(taps, bad, i, prev):
    """the history fetch of flat pixel i over the taps that are not on a bad texel, in float32 and in tap order: prev (n, k) holds the
    previous call's stored values per texel; returns the k fetched values"""
    flat = bad.reshape(-1)
    sw, sums = F(0.0), np.zeros(prev.shape[1], np.float32)
    for valid, j, w in taps:
        if valid[i] and not flat[j[i]]:
            sw = sw + w[i]
            sums = sums + w[i] * prev[j[i]]
    return sums / sw


# ---- the finite sequences behind tests/golden/temporal_finite.npz (make_temporal_finite.py) --------------------------------------------
FINITE_W, FINITE_H, FINITE_CALLS = 32, 20, 3
DENOISE_KEYS = ("color", "temporal", "history", "variance")
TAA_KEYS = ("output", "history")


def finite_denoise(denoiser, flags, motion):
    """three calls of the wall sequence at 32 x 20 with noise in [0, 4] through `denoiser` (a dr.Denoiser or dmr.MotionDenoiser);
    returns {"<call>_<image>": array}"""
    import denoise_reference as dr
    out = {}
    for k in range(FINITE_CALLS):
        c = wall_call(k, FINITE_W, FINITE_H, step=0.3, samples=2)
        acc = wall_noise(k, FINITE_W, FINITE_H, 0.0, 4.0)
        guides = (acc, c["position"], c["normal"], c["albedo"], c["pbr"]) + ((c["motion"],) if motion else ())
        r = denoiser(*guides, c["view"], dr.default_params(flags=flags, iterations=3))
        out.update({f"{k}_{name}": r[name] for name in DENOISE_KEYS})
    return out


def finite_taa(taa, flags):
    out = {}
    for k in range(FINITE_CALLS):
        c = wall_call(k, FINITE_W, FINITE_H, step=0.3)
        pos = c["position"].copy()
        pos[: FINITE_H // 3, :, 3] = 0.0  # the upper third is not geometry: it reprojects its primary ray
        r = taa(wall_noise(k, FINITE_W, FINITE_H, 0.0, 4.0), pos, c["motion"], c["view"], tr.default_params(flags=flags), FINITE_W, FINITE_H)
        out.update({f"{k}_{name}": r[name] for name in TAA_KEYS})
    return out


def finite_denoise_cases(dr, dmr):
    """the denoiser's finite sequences through the given restatement modules: {"<case>/<call>_<image>": array}"""
    out = {}
    for flags in (0, dr.TEMPORAL, dr.DEMODULATE, dr.TEMPORAL | dr.DEMODULATE):
        out.update({f"denoise{flags}/{k}": v for k, v in finite_denoise(dr.Denoiser(), flags, False).items()})
    out.update({f"denoise_motion/{k}": v for k, v in finite_denoise(dmr.MotionDenoiser(), dr.TEMPORAL | dr.DEMODULATE | dmr.MOTION, True).items()})
    return out


def finite_taa_cases(taa_module):
    out = {}
    for flags in (0, taa_module.CLAMP, taa_module.CLAMP | taa_module.MOTION):
        out.update({f"taa{flags}/{k}": v for k, v in finite_taa(taa_module.Taa(), flags).items()})
    return out

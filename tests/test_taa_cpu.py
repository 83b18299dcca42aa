"""CPU: camera.jitter_projection against float64 pixel coordinates, and the restatement of UH_HYBRID_TAA (tests/taa_reference.py) on
synthetic images: known answers that need no device, that a jittered sequence through it anti-aliases an analytic edge, and the rule
for non-finite input ("Non-finite input") on the wall sequence of tests/temporal_cases.py."""
import os

import numpy as np
import pytest

import rust_renderer_amd as rr
import taa_reference as tr
import temporal_cases as tc

F = np.float32
W, H = 40, 24


def rig_camera(w=W, h=H):
    """motion_util.MotionRig's camera"""
    return rr.camera.Camera((0.0, 1.5, 4.0), (0.0, 1.0, -3.0), 60.0, w / h, 0.01, 1000.0)


def projection_view(v):
    proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
    view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
    return tuple((proj @ view).astype(np.float32).T.reshape(-1))


def rest_view(w=W, h=H):
    """the camera at rest: prev_frame_projection_view is its own un-jittered projection * view"""
    v = rr.default_view(rig_camera(w, h), w, h)
    v.prev_frame_projection_view[:] = projection_view(v)
    return v


def pixels64(proj16, view16, pts, w, h):
    """float64 G-buffer pixel coordinates (x right, y down) of world points under column-major matrices"""
    P, V = np.array(proj16, np.float64).reshape(4, 4).T, np.array(view16, np.float64).reshape(4, 4).T
    clip = (P @ V @ np.concatenate([pts, np.ones((len(pts), 1))], axis=1).T).T
    ndc = clip[:, :2] / clip[:, 3:4]
    return np.stack([(ndc[:, 0] * 0.5 + 0.5) * w, (1.0 - (ndc[:, 1] * 0.5 + 0.5)) * h], axis=-1)


# ---- camera.jitter_projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [(0.0, 0.0), (0.25, -0.375), (-0.5, 0.4375), (0.3, 0.2)])
def test_jitter_projection_moves_every_point_by_the_jitter(jitter):
    w, h = 67, 45
    cam = rig_camera(w, h)
    v = rr.default_view(cam, w, h)
    rng = np.random.default_rng(5)
    # in front of the camera (it looks down -z from z = 4): depths 0.5 to 30, anywhere across the frustum and beyond its sides
    pts = np.stack([rng.uniform(-6, 6, 100), rng.uniform(-3, 5, 100), 4.0 - rng.uniform(0.5, 30.0, 100)], axis=-1)
    proj = np.array(v.projection[:], np.float32)
    jp, jinv = rr.camera.jitter_projection(proj, jitter[0], jitter[1], w, h)
    assert jp.dtype == np.float32 and jinv.dtype == np.float32 and jp.shape == (16,) and jinv.shape == (16,)
    if jitter == (0.0, 0.0):
        assert np.array_equal(jp.view(np.uint32), proj.view(np.uint32)), "no jitter: the input's bits"
    moved = pixels64(jp, v.view[:], pts, w, h) - pixels64(proj, v.view[:], pts, w, h)
    assert np.abs(moved - np.array(jitter)).max() <= 1e-4, moved
    ident = jinv.astype(np.float64).reshape(4, 4).T @ jp.astype(np.float64).reshape(4, 4).T
    assert np.abs(ident - np.eye(4)).max() <= 1e-5
    # the Renderer-side convenience applies the same pair to a view struct and touches nothing else
    jv = rr.Renderer.jitter_view(v, 3, w, h)
    want_p, want_i = rr.camera.jitter_projection(proj, *rr.taa_jitter(3), w, h)
    assert np.array_equal(np.array(jv.projection[:], np.float32), want_p) and np.array_equal(np.array(jv.inverse_projection[:], np.float32), want_i)
    assert jv.view[:] == v.view[:] and jv.inverse_view[:] == v.inverse_view[:]
    # and prev_frame_projection_view, un-jittered in the caller's view, gets the same offset: a point lands j from where it did
    v.prev_frame_projection_view[:] = projection_view(v)
    jv = rr.Renderer.jitter_view(v, 3, w, h)
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
    moved = pixels64(jv.prev_frame_projection_view[:], ident, pts, w, h) - pixels64(v.prev_frame_projection_view[:], ident, pts, w, h)
    assert np.abs(moved - np.array(rr.taa_jitter(3))).max() <= 1e-4, moved
    assert np.array_equal(rr.camera.jitter_clip(proj, *jitter, w, h), jp), "on the projection itself jitter_clip is jitter_projection"
    assert v.projection[:] == proj.tolist(), "the caller's view is not changed"


# ---- the restatement on synthetic images -------------------------------------------------------------------------------------------
def half_geometry(v):
    """a position image whose left half is geometry - points 3 to 5 units along each pixel's own primary ray, so that the camera at rest
    reprojects them onto their own texel - and whose right half is not (1, 1, 1, 0)"""
    d = tr.primary_directions(v, W, H).astype(np.float64).reshape(H, W, 3)
    eye = np.array(v.inverse_view[12:15], np.float64)
    t = 3.0 + 2.0 * np.random.default_rng(1).random((H, W, 1))
    pos = np.ones((H, W, 4), np.float32)
    pos[..., :3] = (eye + t * d).astype(np.float32)
    pos[:, W // 2:] = (1.0, 1.0, 1.0, 0.0)
    return pos


def images(n, seed=3):
    rng = np.random.default_rng(seed)
    out = rng.random((n, H, W, 4)).astype(np.float32)
    out[..., 3] = 1.0
    return out


def test_running_mean_bit_for_bit():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    p = tr.default_params(flags=0, alpha_min=0.0, max_history=64)
    x = None
    for n, c in enumerate(images(7), start=1):
        got = taa(c, pos, None, v, p, W, H)
        x = c[..., :3].copy() if x is None else x + (c[..., :3] - x) * (F(1.0) / F(n))  # the float32 recurrence, independently
        assert x.dtype == np.float32
        assert np.array_equal(got["output"][..., :3].view(np.uint32), x.view(np.uint32)), n
        assert np.array_equal(got["output"][..., 3], c[..., 3])
        assert (got["history"] == n).all(), "N is the call count"
        assert got["history_pixels"] == (0 if n == 1 else W * H) and got["reset_pixels"] == W * H - got["history_pixels"]


def test_history_is_capped_and_alpha_min_holds():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    p = tr.default_params(flags=0, alpha_min=0.25, max_history=3)
    x = None
    for n, c in enumerate(images(6, seed=4), start=1):
        got = taa(c, pos, None, v, p, W, H)
        a = max(F(1.0) / F(min(n, 3)), F(0.25))
        x = c[..., :3].copy() if x is None else x + (c[..., :3] - x) * a
        assert np.array_equal(got["output"][..., :3].view(np.uint32), x.view(np.uint32)), n
        assert (got["history"] == min(n, 3)).all()


def test_a_constant_image_comes_back_unchanged_under_the_clamp():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    c = np.empty((H, W, 4), np.float32)
    c[...] = (0.5, 0.25, 2.0, 1.0)  # sums of up to nine of these and their squares are exact in float32: the box is [c, c]
    for n in range(1, 5):
        got = taa(c, pos, None, v, tr.default_params(), W, H)
        assert np.array_equal(got["output"].view(np.uint32), c.view(np.uint32)), n
        assert np.array_equal(got["lo"], c[..., :3]) and np.array_equal(got["hi"], c[..., :3])
        assert (got["history"] == n).all()


def test_the_clamp_is_a_clamp():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    far, near = images(2, seed=8)
    far[..., :3] = far[..., :3] * 5.0 + 10.0  # the history: far above anything in the next frame's boxes
    p = tr.default_params()
    taa(far, pos, None, v, p, W, H)
    got = taa(near, pos, None, v, p, W, H)
    c, out = near[..., :3], got["output"][..., :3]
    assert got["blended"].all()
    assert (far[..., :3].min() > got["hi"].max() + 5.0), "the history lies far outside every box"
    # out = hc + (c - hc) * a with hc in [lo, hi] and a = 1/2: between hc and c
    assert (out >= np.minimum(got["lo"], c)).all() and (out <= np.maximum(got["hi"], c)).all()
    # and the clamp did the work: without it the history shows
    free = tr.Taa()
    free(far, pos, None, v, tr.default_params(flags=0), W, H)
    loose = free(near, pos, None, v, tr.default_params(flags=0), W, H)["output"][..., :3]
    assert (loose > np.maximum(got["hi"], c) + 1.0).all()


def test_reset_starts_every_history_again():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    a, b, c = images(3, seed=9)
    taa(a, pos, None, v, tr.default_params(), W, H)
    assert (taa(b, pos, None, v, tr.default_params(), W, H)["history"] == 2).all()
    taa.reset()
    got = taa(c, pos, None, v, tr.default_params(), W, H)
    assert (got["history"] == 1).all() and got["reset_pixels"] == W * H and got["history_pixels"] == 0
    assert np.array_equal(got["output"], c)


def test_motion_texels_without_a_correspondence_start_again():
    v, taa = rest_view(), tr.Taa()
    pos = half_geometry(v)
    motion = pos.copy()
    motion[:, W // 2:] = 0.0          # not geometry: (0, 0, 0, 0), never read
    motion[: H // 2, : W // 4, 3] = 0.0  # a block of geometry without a correspondence
    p = tr.default_params(flags=tr.MOTION, alpha_min=0.0)
    a, b = images(2, seed=10)
    taa(a, pos, motion, v, p, W, H)
    got = taa(b, pos, motion, v, p, W, H)
    none = np.zeros((H, W), bool)
    none[: H // 2, : W // 4] = True
    assert (got["history"][none] == 1).all() and (got["history"][~none] == 2).all()
    assert np.array_equal(got["output"][none], b[none]) and got["reset_pixels"] == none.sum()


# ---- it anti-aliases: a slanted edge sampled under the jitter sequence ---------------------------------------------------------------
BRIGHT, DARK = np.array([1.0, 0.9, 0.8]), np.array([0.1, 0.1, 0.15])


def scene(x, y):
    """a bright rectangle 22 x 9 pixels, rotated by 0.3 rad about (20.3, 11.6), over a dark ground; x, y continuous pixel coordinates"""
    c, s = np.cos(0.3), np.sin(0.3)
    u, w = (x - 20.3) * c + (y - 11.6) * s, -(x - 20.3) * s + (y - 11.6) * c
    inside = (np.abs(u) <= 11.0) & (np.abs(w) <= 4.5)
    return np.where(inside[..., None], BRIGHT, DARK)


def sampled(jx, jy):
    """the frame of a camera whose projection is jittered by (jx, jy): the image moves by +j, so the centre of pixel p sees what lies at
    p + 0.5 - j of the un-jittered image"""
    y, x = np.mgrid[0:H, 0:W]
    out = np.ones((H, W, 4), np.float32)
    out[..., :3] = scene(x + 0.5 - jx, y + 0.5 - jy)
    return out


def test_a_jittered_sequence_anti_aliases_a_slanted_edge():
    sub = (np.arange(8) + 0.5) / 8.0
    y, x = np.mgrid[0:H, 0:W]
    truth = np.mean([scene(x + sx, y + sy) for sy in sub for sx in sub], axis=0)  # the 8 x 8 supersampled box mean
    plain = sampled(0.0, 0.0)[..., :3].astype(np.float64)
    edge = np.abs(truth - plain).max(axis=-1) > 0.02
    assert edge.sum() >= 40, edge.sum()
    base = rest_view()
    pos = np.tile(np.array([1, 1, 1, 0], np.float32), (H, W, 1))  # no geometry: every pixel reprojects its primary ray's direction
    taa, p = tr.Taa(), tr.default_params()
    errors = []
    for k in range(32):
        v = rr.Renderer.jitter_view(base, k, W, H)  # base holds the un-jittered projection * view: the recipe of INTEGRATION.md
        got = taa(sampled(*rr.taa_jitter(k)), pos, None, v, p, W, H)
        errors.append(float(np.abs(got["output"][..., :3].astype(np.float64) - truth)[edge].mean()))
    unjittered = float(np.abs(plain - truth)[edge].mean())
    print(f"taa on the slanted edge: {edge.sum()} edge pixels, error {errors[15]:.4f} after 16 frames, at most {max(errors[15:]):.4f} over frames 16 to 32, "
          f"un-jittered {unjittered:.4f}")
    assert errors[15] <= 0.5 * unjittered


# ---- non-finite input: a bad pixel passes through and takes part in nothing ("Non-finite input") ---------------
# The wall sequence of temporal_cases.py: call 0 clean, call 1 with the set B planted in the colour image, the calls after it clean.
NONFINITE_FLAGS = [pytest.param(0, id="free"), pytest.param(tr.CLAMP, id="clamp"), pytest.param(tr.CLAMP | tr.MOTION, id="clamp-motion")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def wall_frames(flags, calls):
    """yields (k, result, input image, resolver, the history the call read) for the wall sequence with B planted in call 1"""
    taa, p = tr.Taa(), tr.default_params(flags=flags)
    for k in range(calls):
        c = tc.wall_call(k)
        img = tc.plant(tc.wall_noise(k)) if k == 1 else tc.wall_noise(k)
        before = taa.hist
        yield k, taa(img, c["position"], c["motion"], c["view"], p, tc.W, tc.H), img, taa, before


@pytest.mark.parametrize("flags", NONFINITE_FLAGS)
def test_bad_colours_pass_through_and_reach_no_other_pixel(flags):
    bm, n = tc.b_mask(), tc.W * tc.H
    for k, r, img, taa, before in wall_frames(flags, 3):
        bad_now = bm if k == 1 else np.zeros_like(bm)
        assert np.array_equal(r["bad"], bad_now)
        assert np.isfinite(r["output"][~bad_now]).all() and np.isfinite(r["history"]).all(), k
        assert r["history_pixels"] + r["reset_pixels"] == n and r["history_pixels"] == r["blended"].sum()
        if flags & tr.CLAMP:
            assert np.isfinite(r["lo"][~bad_now]).all() and np.isfinite(r["hi"][~bad_now]).all(), "the boxes leave bad neighbours out"
        if k == 1:
            assert np.array_equal(bits(r["output"][bm]), bits(img[bm])), "the input, bits unchanged"
            assert not r["history"][bm].any() and (r["history"][~bm] >= 1).all(), "0 marks a texel without a history, and only that"
            assert not r["blended"][bm].any(), "B counts in reset_pixels"
            if flags & tr.CLAMP:  # the box beside the interior block, against float64 over the neighbours that are not bad
                x, y = 47, 30
                near = [img[y + dy, x + dx, :3].astype(np.float64) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if not bm[y + dy, x + dx]]
                assert len(near) == 7
                m1, sg = np.mean(near, axis=0), np.std(near, axis=0)
                assert np.abs(r["lo"][y, x] - (m1 - sg)).max() <= 1e-4 and np.abs(r["hi"][y, x] - (m1 + sg)).max() <= 1e-4
        if k == 2:
            only_bad, mixed, clean = tc.tap_kinds(taa.taps, bm)
            assert only_bad.any() and mixed.any() and clean.any(), "all three kinds of pixel exist"
            assert (r["history"][only_bad] == 1).all() and not r["blended"][only_bad].any(), "nothing to fetch: the history starts again"
            assert np.array_equal(bits(r["output"][only_bad]), bits(img[only_bad]))
            assert (r["history"][mixed] == 3).all() and r["blended"][mixed].all() and (r["history"][clean] == 3).all()
            c, out = img.reshape(-1, 4)[:, :3], r["output"].reshape(-1, 4)[:, :3]
            for i in np.flatnonzero(mixed.reshape(-1)):  # renormalised over the taps that remain: the blend from an independent fetch
                prev = tc.renormalised(taa.taps, bm, i, np.concatenate([before[0], before[1][:, None]], axis=1))
                assert prev[3] == 2
                hc = prev[:3]
                if flags & tr.CLAMP:
                    hc = np.minimum(np.maximum(hc, r["lo"].reshape(-1, 3)[i]), r["hi"].reshape(-1, 3)[i])
                assert np.array_equal(bits(out[i]), bits(hc + (c[i] - hc) * (F(1.0) / F(3.0)))), i


# The largest relative excess of an output channel over the hull of the finite inputs so far, measured with the restatement itself on
# these sequences: 0 - hc + (c - hc) * a never left [hc, c], and a clamped hc lies between the fetched one and the box's mean.
TAA_CONVEX_MEASURED = 0.0
TAA_CONVEX_HELD = 4 * TAA_CONVEX_MEASURED


@pytest.mark.parametrize("flags", NONFINITE_FLAGS)
def test_outputs_stay_in_the_hull_of_the_finite_inputs(flags):
    lo, hi, worst = np.full(3, np.inf), np.full(3, -np.inf), -np.inf
    for k, r, img, taa, before in wall_frames(flags, tc.CALLS):
        good = ~r["bad"]
        seen = img[good][:, :3].astype(np.float64)
        lo, hi = np.minimum(lo, seen.min(axis=0)), np.maximum(hi, seen.max(axis=0))
        out = r["output"][good][:, :3].astype(np.float64)
        worst = max(worst, float((np.maximum(out - hi, lo - out) / hi).max()))
    print(f"taa convexity: largest relative excess over the hull {max(worst, 0.0):.3e}")
    assert max(worst, 0.0) <= TAA_CONVEX_HELD


def test_finite_input_gives_the_bits_it_gave_before_the_rule():
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_finite.npz"))
    got = tc.finite_taa_cases(tr)
    assert len(got) == 18 and set(got) <= set(want.files)
    for name, a in got.items():
        assert np.array_equal(bits(a), bits(want[name])), name

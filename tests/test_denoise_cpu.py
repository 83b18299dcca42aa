"""CPU: the numpy restatement of uh_denoise (tests/denoise_reference.py) held to known answers on synthetic arrays - the six cases of
DESIGN.md section 2, "Denoiser". test_gpu_denoise.py runs cases 1, 4, 5 and 6 on the device and holds the device to the restatement. Then the rule for non-finite
input ("Non-finite input") on the wall sequence of tests/temporal_cases.py: containment, that a bad pixel is
treated as one that is not geometry, convexity, and that finite input gives the bits it always gave."""
import os

import numpy as np
import pytest

import denoise_motion_reference as dmr
import denoise_reference as dr
import temporal_cases as tc
import rust_renderer_amd as rr
from hybrid_util import cast_planes, plane_view

F = np.float32
W, H = 40, 24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def projection_view(view):
    """projection * view, column-major, as a caller hands it over in prev_frame_projection_view"""
    m = lambda a: np.array(a[:], np.float64).reshape(4, 4).T
    return tuple((m(view.projection) @ m(view.view)).T.reshape(-1).astype(np.float32))


@pytest.fixture(scope="module")
def floor_frame():
    """a camera above a floor, the upper rows sky: view, position, normal, albedo, pbr"""
    view = plane_view((0.0, 1.5, 4.0), (0.0, 0.5, 0.0), W, H)
    pos, nrm = cast_planes(view, [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))], W, H)
    rng = np.random.default_rng(5)
    alb = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    alb[0, 0, :3] = 0  # the 0.01 floor of the demodulator
    pbr = np.zeros((H, W, 4), np.float32)
    assert (pos[..., 3] == 0).any() and (pos[..., 3] != 0).sum() > W * H // 3
    return view, pos, nrm, alb, pbr


def noise(seed, scale=1.0, shape=(H, W)):
    a = np.zeros(shape + (4,), np.float32)
    a[..., :3] = np.random.default_rng(seed).uniform(0.0, scale, shape + (3,)).astype(np.float32)
    return a


def with_samples(view, n):
    view.total_samples, view.accumulation_limit = n, 999999
    return view


def test_no_levels_no_flags_is_the_input_bit_for_bit(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    acc = noise(1, 3.0)
    r = dr.Denoiser()(acc, pos, nrm, alb, pbr, with_samples(view, 3), dr.default_params(flags=0, iterations=0))
    assert np.array_equal(bits(r["color"]), bits(r["input"]))
    assert np.array_equal(bits(r["input"][..., :3]), bits(acc[..., :3] / F(3.0)))
    assert np.array_equal(r["output"][..., :3][..., ::-1], dr.unorm8(dr.linear_to_srgb(r["color"][..., :3])))
    assert (r["output"][..., 3] == 0).all() and (r["color"][..., 3] == 0).all()


def test_one_level_on_a_plane_cuts_iid_noise_to_the_kernels_energy():
    """every weight is k: normals equal, plane distance 0, sigma_luminance 1e30. Sum of k^2 = (70/256)^2 = 0.0748"""
    n = 112
    y, x = np.mgrid[0:n, 0:n]
    pos = np.stack([x * 0.01, y * 0.01, np.full_like(x, -5.0, dtype=np.float64), np.ones_like(x)], axis=-1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1, 1], np.float32), (n, n, 1))
    view = with_samples(rr.ViewUniformData(), 1)
    view.view[:] = tuple(np.eye(4, dtype=np.float32).reshape(-1))
    acc = np.zeros((n, n, 4), np.float32)
    acc[..., :3] = np.random.default_rng(2).normal(1.0, 0.1, (n, n, 1)).astype(np.float32)
    r = dr.Denoiser()(acc, pos, nrm, np.zeros((n, n, 4), np.uint8), np.zeros((n, n, 4), np.float32), view,
                      dr.default_params(flags=0, iterations=1, sigma_luminance=1e30))
    inner = slice(8, 104)
    ratio = r["color"][inner, inner, 0].astype(np.float64).var() / acc[inner, inner, 0].astype(np.float64).var()
    print("variance ratio", ratio)
    assert abs(ratio / (70.0 / 256.0) ** 2 - 1.0) <= 0.2
    # and the filter's own estimate: var' = sum k^2 var / 1 with a constant var is the same factor of it
    v0, v1 = r["variance"][inner, inner].astype(np.float64), r["final_variance"][inner, inner].astype(np.float64)
    assert np.all(v1 <= v0.max() * (70.0 / 256.0) ** 2 * 1.0001)


@pytest.fixture(scope="module")
def crease():
    """an emissive floor and a black wall at a right angle, both large"""
    view = with_samples(plane_view((0.0, 1.2, 3.0), (0.0, 0.6, -2.0), W, H), 1)
    pos, nrm = cast_planes(view, [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0))], W, H)
    floor, wall = nrm[..., 1] == 1.0, nrm[..., 2] == 1.0
    assert floor.sum() > 100 and wall.sum() > 100 and (floor | wall).all()
    pbr = np.zeros((H, W, 4), np.float32)
    pbr[wall, 3] = 1.0
    acc = noise(3, 2.0)
    acc[wall] = 0.0
    return view, pos, nrm, pbr, acc, floor, wall


def test_no_weight_crosses_a_right_angle(crease):
    view, pos, nrm, pbr, acc, floor, wall = crease
    alb = np.full((H, W, 4), 255, np.uint8)
    r = dr.Denoiser()(acc, pos, nrm, alb, pbr, view, dr.default_params(flags=0))
    assert not bits(r["color"][wall]).any(), "no wall pixel has changed in any bit"
    assert not np.array_equal(bits(r["color"][floor]), bits(r["input"][floor])), "the floor was filtered"
    # a floor pixel is a filter of floor pixels only: whatever the wall's colours are, w_n = 0 multiplies them. (The wall's VARIANCE does
    # reach the 3 x 3 prefilter g of the floor pixels beside it, as the contract says; sigma_luminance = 1e30 takes g out of the weights.)
    p = dr.default_params(flags=0, sigma_luminance=1e30)
    a = dr.Denoiser()(acc, pos, nrm, alb, pbr, view, p)
    acc2 = acc.copy()
    acc2[wall, :3] = np.random.default_rng(9).uniform(0.0, 1e6, (int(wall.sum()), 3)).astype(np.float32)
    b = dr.Denoiser()(acc2, pos, nrm, alb, pbr, view, p)
    assert np.array_equal(bits(a["color"][floor]), bits(b["color"][floor]))
    assert np.isfinite(b["color"]).all()


def test_camera_at_rest_accumulates_the_running_mean(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 1)
    view.prev_frame_projection_view[:] = projection_view(view)
    p = dr.default_params(flags=dr.TEMPORAL, iterations=0, alpha_min=0.0)
    d, k = dr.Denoiser(), 8
    frames = [noise(20 + i, 4.0) for i in range(k)]
    for f in frames:
        r = d(f, pos, nrm, alb, pbr, view, p)
    geo = pos[..., 3] != 0
    assert np.array_equal(r["history"][geo], np.full(int(geo.sum()), F(k))) and not r["history"][~geo].any()
    assert r["kept"][geo].all()
    stack = np.stack([f[..., :3] for f in frames]).astype(np.float64)
    bound = 4 * k * 2.0 ** -23 * stack.max(axis=0)
    err = np.abs(r["temporal"][..., :3].astype(np.float64) - stack.mean(axis=0))
    assert (err[geo] <= bound[geo]).all(), (err[geo] / bound[geo]).max()
    assert np.array_equal(bits(r["temporal"][~geo]), bits(frames[-1][~geo]))


def test_history_off_the_image_and_after_a_reset_is_one(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 1)
    pv = np.array(projection_view(view), np.float32).reshape(4, 4)  # [column][row]
    geo = pos[..., 3] != 0
    p = dr.default_params(iterations=1)
    d = dr.Denoiser()
    view.prev_frame_projection_view[:] = tuple(pv.reshape(-1))
    d(noise(1), pos, nrm, alb, pbr, view, p)
    r = d(noise(2), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 2).all()
    off = pv.copy()
    off[:, 0] += F(10.0) * off[:, 3]  # clip x + 10 w: every point ten half-widths to the right
    view.prev_frame_projection_view[:] = tuple(off.reshape(-1))
    r = d(noise(3), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 1).all() and not r["kept"].any()
    view.prev_frame_projection_view[:] = tuple(pv.reshape(-1))
    assert (d(noise(4), pos, nrm, alb, pbr, view, p)["history"][geo] == 2).all()
    d.reset()
    r = d(noise(5), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 1).all() and not r["kept"].any() and not r["history"][~geo].any()


@pytest.mark.parametrize("flags", [0, dr.TEMPORAL, dr.DEMODULATE, dr.TEMPORAL | dr.DEMODULATE])
def test_pixels_that_are_not_geometry_pass_through_bit_for_bit(floor_frame, flags):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 2)
    view.prev_frame_projection_view[:] = projection_view(view)
    sky = pos[..., 3] == 0
    d = dr.Denoiser()
    for seed in (1, 2):
        acc = noise(seed, 5.0)
        r = d(acc, pos, nrm, alb, pbr, view, dr.default_params(flags=flags))
        want = bits(acc[..., :3] / F(2.0))[sky]
        for name in ("color", "input", "temporal"):
            assert np.array_equal(bits(r[name][..., :3])[sky], want), name
        assert not r["history"][sky].any() and not r["variance"][sky].any()
        assert not np.array_equal(bits(r["color"][~sky]), bits(r["input"][~sky]))


# ---- non-finite input: a bad pixel passes through and takes part in nothing ("Non-finite input") ---------------
# The wall sequence of temporal_cases.py: call 0 clean, call 1 with the set B planted in the accumulation, the calls after it clean.
FLOATS = ("color", "input", "temporal", "history", "variance", "final_variance")
CASES = [pytest.param(0, False, id="plain"), pytest.param(dr.TEMPORAL, False, id="temporal"), pytest.param(dr.DEMODULATE, False, id="demodulate"),
         pytest.param(dr.TEMPORAL | dr.DEMODULATE, False, id="temporal-demodulate"),
         pytest.param(dr.TEMPORAL | dr.DEMODULATE, True, id="temporal-demodulate-motion")]


def wall_calls(flags, motion, calls, edit=None):
    """yields (k, result, acc, denoiser, the history the call read) for the wall sequence; edit(k, acc, call) may change call k's inputs"""
    d = dmr.MotionDenoiser() if motion else dr.Denoiser()
    p = dr.default_params(flags=flags | (dmr.MOTION if motion else 0))
    for k in range(calls):
        c, acc = tc.wall_call(k), tc.wall_noise(k)
        if edit is not None:
            acc = edit(k, acc, c)
        before = d.hist
        guides = (acc, c["position"], c["normal"], c["albedo"], c["pbr"]) + ((c["motion"],) if motion else ())
        yield k, d(*guides, c["view"], p), acc, d, before


def plant_in_call_1(k, acc, c):
    return tc.plant(acc) if k == 1 else acc


@pytest.mark.parametrize("flags,motion", CASES)
def test_bad_samples_pass_through_and_reach_no_other_pixel(flags, motion):
    bm = tc.b_mask()
    for k, r, acc, d, before in wall_calls(flags, motion, 3, plant_in_call_1):
        bad_now = bm if k == 1 else np.zeros_like(bm)
        assert np.array_equal(r["bad"], bad_now) and r["geometry"].all(), "B is geometry (geometry_pixels counts it) and nothing else is bad"
        for name in FLOATS:
            assert np.isfinite(r[name][~bad_now]).all(), (k, name, int((~np.isfinite(r[name])).sum()))
        if k == 1:
            assert not np.isfinite(acc[bm][:, :3]).all(axis=-1).all() and (np.isfinite(acc[bm]).all(axis=-1)).any(), "non-finite and overflowing samples"
            for name in ("color", "input", "temporal"):
                assert np.array_equal(bits(r[name][bm][:, :3]), bits(acc[bm][:, :3])), name  # n = 1: the accumulation's own bits
            assert not r["history"][bm].any() and not r["kept"][bm].any() and not r["variance"][bm].any()
        if k == 2 and flags & dr.TEMPORAL:
            only_bad, mixed, clean = tc.tap_kinds(d.taps, bm)
            assert only_bad.any() and mixed.any() and clean.any(), "all three kinds of pixel exist"
            assert (r["history"][only_bad] == 1).all() and not r["kept"][only_bad].any(), "nothing to fetch: the history starts again"
            assert (r["history"][mixed] == 3).all() and r["kept"][mixed].all() and (r["history"][clean] == 3).all()
            c = r["input"].reshape(-1, 4)[:, :3]
            for i in np.flatnonzero(mixed.reshape(-1)):  # renormalised over the taps that remain: the blend from an independent fetch
                prev = tc.renormalised(d.taps, bm, i, np.concatenate([before["col"], before["N"][:, None]], axis=1))
                assert prev[3] == 2
                want = prev[:3] + (c[i] - prev[:3]) * max(F(1.0) / F(3.0), F(0.2))
                assert np.array_equal(bits(d.hist["col"][i]), bits(want)), i
        elif k == 2:
            assert (r["history"] == 1).all()


@pytest.mark.parametrize("flags,motion", CASES)
def test_a_bad_pixel_is_treated_exactly_as_a_pixel_that_is_not_geometry(flags, motion):
    """the same sequence with B's position texels at w = 0 and finite colours there: outside B every bit is the same, in the call
    with B and in the next"""
    bm = tc.b_mask()
    d2 = dmr.MotionDenoiser() if motion else dr.Denoiser()
    p = dr.default_params(flags=flags | (dmr.MOTION if motion else 0))
    for k, r, acc, d, before in wall_calls(flags, motion, 3, plant_in_call_1):
        c, acc2 = tc.wall_call(k), tc.wall_noise(k)
        if k == 1:
            c["position"][bm, 3] = 0.0
        guides = (acc2, c["position"], c["normal"], c["albedo"], c["pbr"]) + ((c["motion"],) if motion else ())
        r2 = d2(*guides, c["view"], p)
        assert not r2["bad"].any() and np.isfinite(r2["color"]).all()
        outside = ~bm if k == 1 else np.ones_like(bm)
        for name in FLOATS:
            assert np.array_equal(bits(r[name])[outside], bits(r2[name])[outside]), (k, name)
        assert np.array_equal(r["kept"], r2["kept"]) and np.array_equal(r["output"][outside], r2["output"][outside])


# The largest relative excess of a filtered channel over the hull of the inputs, measured on these sequences with the restatement
# itself: 0 without DEMODULATE, 3.030e-08 with it alone, 2.235e-08 with TEMPORAL as well (with and without MOTION) - the rounding of
# the division by dm and the product with it again; the normalised sums themselves never left the hull here.
CONVEX_MEASURED = 3.030e-08
CONVEX_HELD = 4 * CONVEX_MEASURED


@pytest.mark.parametrize("flags,motion", CASES)
def test_outputs_stay_in_the_hull_of_the_finite_inputs(flags, motion):
    bm = tc.b_mask()
    lo, hi, worst = np.full(3, np.inf), np.full(3, -np.inf), 0.0
    for k, r, acc, d, before in wall_calls(flags, motion, tc.CALLS, plant_in_call_1):
        good = ~r["bad"]
        seen = r["input"][good][:, :3].astype(np.float64)  # demodulated where the flag is set
        assert np.isfinite(seen).all()
        lo, hi = np.minimum(lo, seen.min(axis=0)), np.maximum(hi, seen.max(axis=0))
        dm = np.ones((tc.H, tc.W, 3))
        if flags & dr.DEMODULATE:
            dm = np.maximum(tc.wall_call(k)["albedo"][..., :3].astype(np.float32) / F(255.0), F(0.01)).astype(np.float64)
        for name in ("temporal", "color"):  # both remodulated: the hull scales by the pixel's own dm
            out = r[name][..., :3].astype(np.float64)
            excess = np.maximum(out - hi * dm, lo * dm - out) / (hi * dm)
            worst = max(worst, float(excess[good].max()))
    print(f"convexity: largest relative excess over the hull {worst:.3e}")
    assert worst <= CONVEX_HELD


def test_finite_input_gives_the_bits_it_gave_before_the_rule():
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_finite.npz"))
    got = tc.finite_denoise_cases(dr, dmr)
    assert len(got) == 60 and set(got) <= set(want.files)
    for name, a in got.items():
        assert np.array_equal(bits(a), bits(want[name])), name

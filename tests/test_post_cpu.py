"""CPU: known answers on tests/post_reference.py, the numpy restatement of the HDR display chain (UH_HYBRID_POST). None of them compares
the restatement with itself: each holds it to a value worked out another way - a float64 geometric mean, a constant image, the clamps,
0.5 - so that the bit-for-bit GPU tests of tests/test_gpu_post.py compare the device with something that is known to be right."""
import numpy as np
import pytest

import post_reference as pr

F = np.float32


def grey(lum, alpha=1.0):
    """an (H, W, 4) image whose three channels are `lum`"""
    lum = np.asarray(lum, F)
    return np.stack([lum, lum, lum, np.full_like(lum, alpha)], axis=-1)


def log_uniform(rng, shape, lo, hi):
    return np.exp2(rng.uniform(lo, hi, size=shape)).astype(F)


def constant(W, H, rgb):
    img = np.empty((H, W, 4), F)
    img[..., :3], img[..., 3] = np.asarray(rgb, F), 1.0
    return img


# ---- metering -------------------------------------------------------------------------------------------------------------------------
def test_metering_is_within_the_derived_bound_of_the_geometric_mean():
    """|log2(Lavg / G)| <= 0.0861 + 0.0625: max(log2(1 + m) - m) = 0.0861 covers the piecewise-linear log and its inverse, half a bin of
    1/8 octave the 0.0625. Measured here over the 40 images below: the worst is printed."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(40):
        lo = rng.uniform(-14.0, 10.0)
        hi = rng.uniform(lo + 0.5, 15.0)
        img = grey(log_uniform(rng, (48, 64), lo, hi))
        hist = pr.histogram(img)
        assert hist[0] == 0 and hist.sum() == 48 * 64
        lavg, n = pr.metered_average(hist, 0.0, 1.0)
        L = pr.luminance(img[..., :3]).astype(np.float64)
        G = np.exp2(np.log2(L).mean())
        assert n == 48 * 64
        err = abs(np.log2(float(lavg) / G))
        worst = max(worst, err)
        assert err <= 0.0861 + 0.0625, (k, err)
    print("worst |log2(Lavg / G)|:", worst)


def test_a_constant_image_meters_into_one_bin():
    for v in (2.0 ** -15.5, 0.18, 1.0, 3.7, 30000.0):
        hist = pr.histogram(grey(np.full((9, 13), v)))
        assert (hist != 0).sum() == 1 and hist.max() == 9 * 13 and hist[0] == 0
        L = float(pr.luminance(grey(np.full((1, 1), v))[..., :3])[0, 0])
        e = int(np.floor(np.log2(L)))  # eight bins per octave from 2^-16, linear in the mantissa inside an octave
        assert np.argmax(hist) == (e + 16) * 8 + int(np.floor((L / 2.0 ** e - 1.0) * 8.0))
    # below the first bin's octave, at or below 0, NaN and bad: bin 0, or bin 1's floor for the tiny positive ones
    odd = grey(np.array([[0.0, -1.0, np.nan, np.inf, 2.0 ** 49]], F))
    assert pr.histogram(odd)[0] == 5
    assert pr.histogram(grey(np.full((2, 2), 2.0 ** -30)))[0] == 4, "below 2^-16 clamps into bin 0, which is not metered"


def test_trimming_ignores_four_percent_of_outliers():
    base, hot = 0.25, 250.0
    with_hot = np.full(1000, base, F)
    with_hot[::25] = hot  # 40 of 1000
    a = pr.metered_average(pr.histogram(grey(with_hot.reshape(25, 40))), 0.5, 0.95)
    b = pr.metered_average(pr.histogram(grey(np.full((24, 40), base, F))), 0.5, 0.95)
    assert a[0] == b[0] and (a[1], b[1]) == (1000, 960)
    untrimmed = pr.metered_average(pr.histogram(grey(with_hot.reshape(25, 40))), 0.0, 1.0)
    assert untrimmed[0] > a[0], "without the percentiles the outliers raise the mean"


def test_exposure_stays_inside_its_clamps_and_nothing_metered_keeps_the_previous():
    rng = np.random.default_rng(3)
    p = pr.params(min_exposure=0.25, max_exposure=8.0)
    hit = set()
    for e in (-15.0, -8.0, -2.0, 0.0, 3.0, 9.0, 14.0):
        img = grey(log_uniform(rng, (16, 16), e, e + 0.9))
        E, target, lavg, n = pr.exposure(pr.histogram(img), p, None)
        assert F(0.25) <= target <= F(8.0) and E == target and n == 256
        hit.add(float(target))
    assert {0.25, 8.0} <= hit and len(hit) > 2, "both clamps and the range between them are exercised"
    black = pr.histogram(grey(np.zeros((4, 4))))
    assert pr.exposure(black, p, F(3.5))[:2] == (F(3.5), F(3.5)) and pr.exposure(black, p, None)[0] == p["manual_exposure"]
    assert pr.exposure(None, pr.params(manual_exposure=2.5), F(7.0))[0] == F(2.5), "without the flag: manual_exposure"


def test_adaptation_approaches_the_target_monotonically():
    img = grey(np.full((8, 8), 0.02))
    for start in (F(0.015625), F(64.0)):
        post, p = pr.Post(), pr.params(adaptation=0.25)
        post.E = start
        target = pr.exposure(pr.histogram(img), p, None)[1]
        gaps = []
        for _ in range(40):
            r = post(img, p)
            assert r["target"] == target
            gaps.append(abs(float(r["exposure"]) - float(target)))
        assert all(b <= a for a, b in zip(gaps, gaps[1:])) and gaps[-1] < 1e-3 * float(target) + 1e-4 and gaps[0] > gaps[-1]
        assert (float(start) - float(target)) * (float(post.E) - float(target)) >= 0, "it never crosses its target"
    post, p = pr.Post(), pr.params(adaptation=1.0)
    post.E = F(0.3)
    r = post(img, p)
    assert abs(float(r["exposure"]) - float(r["target"])) <= float(np.spacing(max(F(0.3), r["target"]))), "there after one call, to rounding"
    post.reset()
    assert post(img, pr.params())["exposure"] == r["target"], "after a reset the pass snaps"


# ---- bloom ----------------------------------------------------------------------------------------------------------------------------
def test_level_sizes_follow_the_ceil_rule():
    assert pr.level_size(1, 1, 0) == (1, 1) and pr.level_size(1, 1, 1) is None and pr.level_count(1, 1, 8) == 0
    assert [pr.level_size(97, 61, k) for k in range(9)] == [(97, 61), (49, 31), (25, 16), (13, 8), (7, 4), (4, 2), (2, 1), (1, 1), None]
    assert pr.level_count(97, 61, 8) == 7 and pr.level_count(97, 61, 3) == 3
    assert [pr.level_size(1, 45, k) for k in range(1, 8)] == [(1, 23), (1, 12), (1, 6), (1, 3), (1, 2), (1, 1), None]
    assert pr.level_size(1920, 1080, 8) == (8, 5) and pr.level_size(4, 4, 9) is None


@pytest.mark.parametrize("size", pr.SIZES + [(2, 2), (128, 8)])
def test_bloom_of_a_constant_image(size):
    """both filters' weights are dyadic and sum to 1, so a constant maps to itself - exactly, for a constant whose partial sums k c / 64
    are representable (the values here have four mantissa bits)"""
    W, H = size
    p = pr.params(bloom_levels=8)
    dn, up = pr.bloom(constant(W, H, (0.75, 0.5, 0.25)), F(1.0), p)  # below the threshold 1.0
    assert len(dn) == pr.level_count(W, H, 8)
    assert all((d == 0).all() and (up[k] == 0).all() for k, d in dn.items())
    dn, up = pr.bloom(constant(W, H, (2.0, 1.0, 0.5)), F(2.0), p)  # exposed (4, 2, 1): m = 4, scaled by 0.75
    for k, d in dn.items():
        assert d.shape == pr.level_size(W, H, k)[::-1] + (3,)
        assert (d == np.array([3.0, 1.5, 0.75], F)).all() and (up[k] == np.array([3.0, 1.5, 0.75], F)).all(), k
    if (W, H) == (1, 1):
        out = pr.evaluate(constant(1, 1, (2.0, 1.0, 0.5)), pr.params(tonemap=pr.NONE), F(2.0))["output"]
        assert (out[0, 0] == np.array([4.0, 2.0, 1.0, 1.0], F)).all(), "no level: bloom is 0"


def test_a_single_bright_texel_spreads_and_conserves_its_sum():
    """the down filter's weights sum to 1 over the destination too (away from the border): the pyramid keeps a texel's energy / 4 per level"""
    img = constant(33, 33, (0.0, 0.0, 0.0))
    img[16, 16, :3] = (5.0, 3.0, 2.0)
    dn, up = pr.bloom(img, F(1.0), pr.params(bloom_levels=2))
    pre = np.array([5.0, 3.0, 2.0]) * 0.8
    assert np.allclose(dn[1].sum(axis=(0, 1)), pre / 4, rtol=1e-6) and np.allclose(dn[2].sum(axis=(0, 1)), pre / 16, rtol=1e-6)
    assert (dn[1] >= 0).all() and (dn[1] > 0).sum() == 3 * 4


# ---- operators ------------------------------------------------------------------------------------------------------------------------
def test_operators():
    one = np.array([1.0], F)
    assert pr.tonemap(one, pr.REINHARD)[0] == F(0.5)
    x = np.concatenate([[0.0], np.exp2(np.linspace(-24.0, 20.0, 20001))]).astype(F)
    for op in (pr.REINHARD, pr.ACES):
        y = pr.tonemap(x, op)
        assert (np.diff(y) >= 0).all() and y.min() >= 0 and y.max() <= 1 and y[0] <= F(0.01), op
        huge = pr.tonemap(np.array([2.0 ** 64, -2.0 ** 64, -0.0], F), op)
        assert np.isfinite(huge).all() and huge[1] == 0 and not np.signbit(huge[2]), op
    assert pr.tonemap(np.array([2.0 ** 20], F), pr.ACES)[0] == F(1.0)
    big = np.array([2.0 ** 64], F)
    assert pr.tonemap(big, pr.NONE)[0] == big[0]


def test_pass_through_setting_returns_the_source_bit_for_bit():
    rng = np.random.default_rng(11)
    img = (log_uniform(rng, (13, 17, 4), -20, 20) * rng.choice([-1.0, 1.0], size=(13, 17, 4))).astype(F)
    img[2, 3, 0], img[4, 5, 1], img[6, 7, 2], img[0, 0, :3] = np.nan, np.inf, 2.0 ** 49, -0.0
    out = pr.Post()(img, pr.params(flags=0, tonemap=pr.NONE, manual_exposure=1.0))["output"]
    assert np.array_equal(out.view(np.uint32), img.view(np.uint32))


def test_bad_pixels_pass_through_and_every_other_texel_is_finite():
    rng = np.random.default_rng(5)
    img = log_uniform(rng, (20, 31, 4), -6, 6)
    badv = [np.nan, np.inf, -np.inf, np.nextafter(F(2.0 ** 48), F(np.inf))]
    for k, v in enumerate(badv):
        img[3 + 4 * k, 5 + k, k % 3] = v
    img[10, 10, 0] = img[10, 11, 1] = np.nan  # adjacent
    img[15, 15, :3] = 2.0 ** 48  # the bound itself is good
    for op in (pr.NONE, pr.REINHARD, pr.ACES):
        r = pr.Post()(img, pr.params(tonemap=op, max_exposure=65536.0, key=65536.0))
        bad = pr.bad_mask(img)
        assert bad.sum() == 6 == r["bad"] and not bad[15, 15]
        assert np.array_equal(r["output"].view(np.uint32)[bad], img.view(np.uint32)[bad])
        assert np.isfinite(r["output"][~bad]).all() and all(np.isfinite(d).all() for d in r["down"].values())
        assert r["metered"] == 20 * 31 - 6


def ulps(a, b):
    """distance in float32 units in the last place (finite values of one sign)"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- rounding -------------------------------------------------------------------------------------------------------------------------
ROUNDING_ULP = 16  # measured: see the docstring below


@pytest.mark.parametrize("op", [pr.NONE, pr.REINHARD, pr.ACES])
def test_float32_stays_close_to_float64(op):
    """The float32 restatement against the same formulas in float64 at the same exposure, on the metering images (log-uniform luminance
    inside [2^-14, 2^15], positive, so that no sum cancels) at every size of the list, all eight levels: measured 4 ulp of the output
    for NONE, 3 for Reinhard, 4 for ACES. A texel where the float64 prefilter decides m > threshold the other way than float32 would
    differ by the whole bloom term; none of the images below has one. The bound is four times the measured worst."""
    rng = np.random.default_rng(19)
    worst = 0
    for W, H in pr.SIZES:
        img = grey(log_uniform(rng, (H, W), -14.0, 15.0))
        img[..., 1] *= F(0.5)
        p = pr.params(tonemap=op, bloom_levels=8, bloom_intensity=0.25)
        E = pr.exposure(pr.histogram(img), p, None)[0]
        a, b = pr.evaluate(img, p, E), pr.evaluate(img, p, E, np.float64)
        worst = max(worst, int(ulps(a["output"], b["output"]).max()))
    print("operator", op, "worst ulp:", worst)
    assert worst <= ROUNDING_ULP

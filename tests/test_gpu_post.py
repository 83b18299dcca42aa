"""GPU: the HDR display chain (UH_HYBRID_POST, uh_post_image) against the numpy restatement of tests/post_reference.py, bit for bit: the
histogram, the exposure record, every bloom level and post_output, on chosen images through uh_post_image at the hybrid size list and in
the hybrid frame of the synthetic scene; exposure over call sequences, the refusals of uh_set_post_params, that the bit changes nothing
else, and that two fresh contexts agree."""
import ctypes as C

import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_util as hu
import post_reference as pr
import rust_renderer_amd as rr
from hybrid_util import bits
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

F = np.float32
OPERATORS = (rr.TONEMAP_NONE, rr.TONEMAP_REINHARD, rr.TONEMAP_ACES)
NEXT_ABOVE = np.nextafter(F(2.0 ** 48), F(np.inf))


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def noise(W, H, seed, lo=-20.0, hi=20.0, negative=0.2):
    """log-uniform values across 2^lo..2^hi, a share of the channels negative"""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(lo, hi, size=(H, W, 4))).astype(F)
    img[rng.random((H, W, 4)) < negative] *= F(-1.0)
    return img


def constant(W, H):
    img = np.empty((H, W, 4), F)
    img[...] = (3.0, 1.7, 0.4, 0.5)
    return img


def corners(W, H):
    """a dim frame with one bright texel in each corner and at the centre: the clamped taps"""
    img = np.empty((H, W, 4), F)
    img[...] = (0.05, 0.04, 0.03, 1.0)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        img[y, x, :3] = (40.0 + x, 25.0, 9.0 + y)
    return img


def with_bad(W, H):
    """noise with NaN, +-inf, 2^48 (good) and the next float above it (bad), isolated and adjacent, wherever the frame has room"""
    img = noise(W, H, 4, -6.0, 6.0, 0.0)
    flat = img.reshape(-1, 4)
    n = flat.shape[0]
    values = [np.nan, np.inf, -np.inf, NEXT_ABOVE, -NEXT_ABOVE, np.nan, np.nan]
    places = [0, n // 7, 2 * n // 7, 3 * n // 7, 4 * n // 7, 5 * n // 7, 5 * n // 7 + 1]  # the last two adjacent
    for k, (at, v) in enumerate(zip(places, values)):
        flat[min(at, n - 1), k % 3] = v
    flat[n - 1, :3] = 2.0 ** 48 if n > 8 else flat[n - 1, :3]
    return img


IMAGES = dict(noise=lambda W, H: noise(W, H, 1), constant=constant, corners=corners, bad=with_bad)


# ---- renderers and the comparison -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare():
    """a renderer without a scene per frame size: uh_post_image needs none"""
    made = {}

    def get(size):
        if size not in made:
            made[size] = rr.Renderer(*size)
        return made[size]

    yield get
    for r in made.values():
        r.close()


def f32(x):
    return np.array([x], F).view(np.uint32)[0]


def hold(gpu, want, src):
    """everything the last pass left on the device against `want` (post_reference.Post's result) for the source image `src`"""
    W, H = gpu.width, gpu.height
    s = gpu.post_stats()
    got = (f32(s.exposure), f32(s.target_exposure), f32(s.average_luminance), s.metered_pixels, s.bad_pixels, s.levels)
    assert got == (f32(want["exposure"]), f32(want["target"]), f32(want["lavg"]), want["metered"], want["bad"], want["levels"])
    if want["histogram"] is None:
        with pytest.raises(UtopianError, match="took no histogram"):
            gpu.read_post(rr.POST_HISTOGRAM)
    else:
        assert np.array_equal(gpu.read_post(rr.POST_HISTOGRAM), want["histogram"])
    for k in range(1, want["levels"] + 1):
        for which, name in ((rr.POST_BLOOM_DOWN, "down"), (rr.POST_BLOOM_UP, "up")):
            img = gpu.read_post(which, k)
            assert img.shape[:2] == want[name][k].shape[:2] == pr.level_size(W, H, k)[::-1]
            assert np.array_equal(bits(img[..., :3]), bits(want[name][k])), (name, k)
            assert (bits(img[..., 3]) == 0).all(), "bloom images have alpha 0"
    if pr.level_size(W, H, want["levels"] + 1) is not None:  # the frame has the level, the pass did not build it
        with pytest.raises(UtopianError, match="did not build"):
            gpu.read_post(rr.POST_BLOOM_DOWN, want["levels"] + 1)
    else:  # the Python layer knows no size to read it at
        with pytest.raises(ValueError, match="no bloom level"):
            gpu.read_post(rr.POST_BLOOM_UP, want["levels"] + 1)
    out = gpu.read_post(rr.POST_OUTPUT)
    assert np.array_equal(bits(out), bits(want["output"]))
    bad = pr.bad_mask(src)
    assert np.array_equal(bits(out)[bad], bits(src)[bad]) and np.isfinite(out[~bad]).all()
    return out


# ---- 1. bit for bit through uh_post_image ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(IMAGES))
@pytest.mark.parametrize("size", pr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_restatement(bare, size, kind):
    gpu = bare(size)
    img = IMAGES[kind](*size)
    for op in OPERATORS:
        for flags in (0, rr.POST_AUTO_EXPOSURE, rr.POST_BLOOM, rr.POST_AUTO_EXPOSURE | rr.POST_BLOOM):
            p = gpu.set_post_params(flags=flags, tonemap=op, bloom_levels=8, manual_exposure=1.5, bloom_intensity=0.25, adaptation=0.5)
            gpu.reset_post_exposure()
            ref = pr.Post()
            for call in range(2):  # the second call adapts from the first's exposure
                gpu.post_image(img if call == 0 else img * F(4.0))
                want = ref(img if call == 0 else img * F(4.0), pr.params_of(p))
                hold(gpu, want, img if call == 0 else img * F(4.0))
            assert want["levels"] == (pr.level_count(*size, 8) if flags & rr.POST_BLOOM else 0)


def test_default_params_on_a_frame_of_several_blocks(bare):
    """the defaults (six levels, trimming percentiles) on a frame wider than one block row, bad pixels included"""
    gpu = bare((257, 3))
    p = gpu.set_post_params()
    gpu.reset_post_exposure()
    ref = pr.Post()
    for seed in (2, 3):
        img = noise(257, 3, seed, -8.0, 8.0)
        img[1, 100 + seed, 0] = np.nan
        gpu.post_image(img)
        want = hold(gpu, ref(img, pr.params_of(p)), img)
    assert gpu.post_stats().levels == 6 and gpu.post_stats().renders > 0 and want is not None


# ---- 2. sequences ---------------------------------------------------------------------------------------------------------------------
def test_exposure_history_reset_and_refused_params(bare):
    size = (97, 61)
    gpu = bare(size)
    p = gpu.set_post_params(adaptation=0.25, bloom_levels=3)
    gpu.reset_post_exposure()
    ref, history = pr.Post(), []
    for k, scale in enumerate((1.0, 30.0, 0.02)):
        img = noise(*size, 10 + k, -3.0, 3.0) * F(scale)
        gpu.post_image(img)
        want = ref(img, pr.params_of(p))
        hold(gpu, want, img)
        history.append((float(want["exposure"]), float(want["target"])))
    assert history[0][0] == history[0][1], "the first pass snaps"
    assert all(e != t for e, t in history[1:]) and len({t for _, t in history}) == 3, "the later ones adapt toward moving targets"
    gpu.reset_post_exposure()
    ref.reset()
    gpu.post_image(img)
    want = ref(img, pr.params_of(p))
    hold(gpu, want, img)
    assert gpu.post_stats().exposure == gpu.post_stats().target_exposure == history[2][1], "after the reset the pass snaps to its target"
    # all-black: nothing metered, the exposure stays
    black = np.zeros((61, 97, 4), F)
    gpu.post_image(black)
    hold(gpu, ref(black, pr.params_of(p)), black)
    assert gpu.post_stats().metered_pixels == 0 and gpu.post_stats().exposure == F(history[2][1])
    # one case per refusal: the message, and the old params stay in force
    nan = float("nan")
    for bad, why in ((dict(flags=4), "unknown flag bits"), (dict(tonemap=3), "tonemap must be 0..2"), (dict(bloom_levels=0), "bloom_levels must be 1..8"),
                     (dict(bloom_levels=9), "bloom_levels must be 1..8"), (dict(manual_exposure=0.0), "must be finite and in (0, 65536]"),
                     (dict(key=nan), "must be finite and in (0, 65536]"), (dict(min_exposure=float("inf")), "must be finite and in (0, 65536]"),
                     (dict(max_exposure=65537.0), "must be finite and in (0, 65536]"), (dict(min_exposure=2.0, max_exposure=1.0), "must not exceed"),
                     (dict(adaptation=0.0), "adaptation must be in (0, 1]"), (dict(adaptation=1.5), "adaptation must be in (0, 1]"),
                     (dict(low_percentile=0.5, high_percentile=0.5), "percentiles must be"), (dict(low_percentile=-0.1), "percentiles must be"),
                     (dict(high_percentile=1.5), "percentiles must be"), (dict(bloom_threshold=-1.0), "bloom_threshold and bloom_intensity"),
                     (dict(bloom_intensity=nan), "bloom_threshold and bloom_intensity")):
        with pytest.raises(UtopianError) as e:
            gpu.set_post_params(**bad)
        assert why in str(e.value) and "uh_set_post_params" in str(e.value), (bad, str(e.value))
    img = noise(*size, 20, -3.0, 3.0)
    gpu.post_image(img)
    hold(gpu, ref(img, pr.params_of(p)), img)


# ---- 3. in the frame ------------------------------------------------------------------------------------------------------------------
class FrameRig:
    """the synthetic scene of hybrid_util.py on a renderer of its own"""

    def __init__(self, size):
        self.size = size
        self.scene = hu.synthetic_scene()
        self.gpu = rr.Renderer(*size)
        self.scene.upload(self.gpu)

    def view(self, fxaa=0):
        v = hu.frame_view(self.scene, *self.size)
        v.num_lights = self.gpu.get_num_lights()
        v.fxaa_enabled = fxaa
        pv = (np.array(v.projection[:], F).reshape(4, 4).T @ np.array(v.view[:], F).reshape(4, 4).T).T.reshape(16)
        v.prev_frame_projection_view[:] = pv.tolist()
        return v


@pytest.mark.parametrize("size", [(97, 61), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_pass_in_the_frame(size):
    r = FrameRig(size)
    g = r.gpu
    p = g.set_post_params(bloom_levels=4, key=0.5, bloom_threshold=0.25)
    ref = pr.Post()
    for fxaa in (0, 1):
        g.render_hybrid(r.view(fxaa), rr.HYBRID_FRAME | rr.HYBRID_POST)
        d = g.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        out = hold(g, ref(d, pr.params_of(p)), d)
        assert g.post_stats().levels == 4 and g.post_stats().metered_pixels > 0
        assert np.array_equal(g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), fr.present(out, bool(fxaa))), fxaa
        assert not np.array_equal(g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), fr.present(d, bool(fxaa))), "present shows the chain"
    # with the taa pass in the same call the source is taa_output (the second taa pass blends a history: it differs from deferred_output)
    for call in range(2):
        g.render_hybrid(r.view(0), rr.HYBRID_FRAME | rr.HYBRID_TAA | rr.HYBRID_POST)
        t = g.read_hybrid(rr.HYBRID_TAA_OUTPUT)
        out = hold(g, ref(t, pr.params_of(p)), t)
        assert np.array_equal(g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), fr.present(out, False))
    # the pass-through setting: present is what it is without the bit
    g.set_post_params(flags=0, tonemap=rr.TONEMAP_NONE, manual_exposure=1.0)
    for fxaa in (0, 1):
        g.render_hybrid(r.view(fxaa), rr.HYBRID_FRAME | rr.HYBRID_POST)
        with_bit = g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
        assert np.array_equal(bits(g.read_post(rr.POST_OUTPUT)), bits(g.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)))
        g.render_hybrid(r.view(fxaa), rr.HYBRID_FRAME)
        assert np.array_equal(with_bit, g.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)), fxaa
    g.close()


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------
def _integers(s):
    """the integer fields of a stats structure (arrays as lists): its counters, not its times"""
    out = {}
    for name, ctype in s._fields_:
        base = getattr(ctype, "_type_", ctype) if hasattr(ctype, "_length_") else ctype
        if base in (C.c_uint32, C.c_uint64, C.c_int32, C.c_int64):
            v = getattr(s, name)
            out[name] = list(v) if hasattr(ctype, "_length_") else v
    return out


def test_the_bit_changes_nothing_else():
    size = (97, 61)
    plain, post = FrameRig(size), FrameRig(size)
    assert bytes(plain.gpu.post_stats()) == bytes(48), "all zero before the first pass"
    buf = np.empty((61, 97, 4), F)
    readable = 0
    for step in range(2):
        mask = rr.HYBRID_FRAME | rr.HYBRID_MOTION | rr.HYBRID_TAA
        plain.gpu.render_hybrid(plain.view(1), mask)
        post.gpu.render_hybrid(post.view(1), mask | rr.HYBRID_POST)
        for which in range(18):
            if which == rr.HYBRID_PRESENT_OUTPUT:
                continue
            bufs = [np.zeros((61, 97, 4), F), np.zeros((61, 97, 4), F)]
            status = [g._api.read_hybrid(g._ctx, which, b.ctypes.data) for g, b in zip((plain.gpu, post.gpu), bufs)]
            assert status[0] == status[1], (which, status)  # (the images of passes that never ran are refused on both)
            assert np.array_equal(bits(bufs[0]), bits(bufs[1])), (step, which)
            readable += status[0] == 0
        assert not np.array_equal(plain.gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), post.gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT))
        sa, sb = plain.gpu.hybrid_frame_stats(), post.gpu.hybrid_frame_stats()
        assert (sa.sky_pixels, sa.lights) == (sb.sky_pixels, sb.lights) and sa.sky_pixels > 0
        assert all((x > 0) == (y > 0) for x, y in zip(sa.pass_ms, sb.pass_ms)), "the same passes ran"
        assert _integers(plain.gpu.get_stats()) == _integers(post.gpu.get_stats())
        ta, tb = plain.gpu.taa_stats(), post.gpu.taa_stats()
        assert (ta.history_pixels, ta.reset_pixels) == (tb.history_pixels, tb.reset_pixels)
    assert readable == 2 * 11, "images 0..7 and 15..17 were compared in both steps"
    # the context that never set the bit: zero stats, no read-back; the one that did: times for its stages only
    assert bytes(plain.gpu.post_stats()) == bytes(48)
    with pytest.raises(UtopianError, match="before the first post pass"):
        plain.gpu.read_post(rr.POST_OUTPUT)
    s = post.gpu.post_stats()
    assert s.renders == 2 and s.meter_ms > 0 and s.bloom_ms > 0 and s.tonemap_ms > 0
    # uh_read_hybrid keeps its indices (this holds without the feature too: it guards the existing contract)
    for g in (plain.gpu, post.gpu):
        assert g._api.read_hybrid(g._ctx, 18, buf.ctypes.data) == 1 and b"0..17" in g._lib.uh_last_error(g._ctx)
    # bit 9 is still ignored
    post.gpu.render_hybrid(post.view(1), rr.HYBRID_FRAME | 1 << 9)
    assert post.gpu.post_stats().renders == 2
    plain.gpu.close(), post.gpu.close()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
def test_two_fresh_contexts_agree():
    img = noise(97, 61, 30, -10.0, 10.0)
    results = []
    for _ in range(2):
        g = rr.Renderer(97, 61)
        g.post_image(img)
        n = g.post_stats().levels
        results.append([g.read_post(rr.POST_HISTOGRAM), g.read_post(rr.POST_OUTPUT)] + [g.read_post(w, k) for w in (rr.POST_BLOOM_DOWN, rr.POST_BLOOM_UP) for k in range(1, n + 1)])
        g.close()
    assert len(results[0]) == 2 + 2 * 6
    for a, b in zip(*results):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))

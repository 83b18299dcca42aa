"""GPU: one-bounce ray-traced diffuse GI of the hybrid frame (uh_render_hybrid's UH_HYBRID_RTGI) against the restatement of
tests/rtgi_reference.py on the device's own G-buffer, ssao image and deferred output: the ray counts byte for byte with the pass's totals,
the radiance image and the composited deferred output bit for bit wherever no missed ray enters (and within the sky's tolerance where
one does), known answers (a bare floor under the furnace, the inside of a closed box, the sky alone), isolation, the refusals in their
order, determinism, and the frame with TAA and the display chain behind it."""
import numpy as np
import pytest

import rtgi_reference as gi
import rust_renderer_amd as rr
from hybrid_util import bits, gbuf, pair, read_all
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

W, H = gi.W, gi.H
RTGI = rr.HYBRID_RTGI
RADIANCE, COUNTS = rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS
FRAME = rr.HYBRID_FRAME | RTGI
# what hybrid_util.check_frame grants the sky pass's pixels of deferred_output (np.allclose(got, want, rtol=1e-4, atol=1e-6)): the device's
# IntegrateScattering against the oracle's
SKY_RTOL, SKY_ATOL = 1e-4, 1e-6


def integers(s):
    return (s.pixels, s.rays, s.shadow_rays, s.misses)


class World:
    """a scene on a GPU renderer and on the oracle; the restatement's rays of a view are computed once per (samples, furnace, frame number)
    on the device's G-buffer and shared by the checks that follow (the G-buffer is compared before they are reused)"""

    def __init__(self, scene, width=W, height=H, on=None):
        """on: (GPU renderer, oracle, mesh records) that hold the scene already, instead of an upload of `scene`"""
        self.scene, self.size = scene, (width, height)
        self.gpu, self.cpu, self.meshes = on if on is not None else pair(scene, width, height)
        self._gathered = {}

    def set_oracle(self, cpu, meshes):
        """another oracle and its mesh records (the geometry changed): the shared rays are forgotten"""
        self.cpu, self.meshes = cpu, meshes
        self.forget()

    def forget(self):
        """the shared rays were made for geometry that has changed since (their key does not know it)"""
        self._gathered = {}

    def set_params(self, **params):
        self.params = gi.default_params(**params)
        self.gpu.set_rtgi_params(**self.params)

    def view(self, **kw):
        return gi.scene_view(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        """a G-buffer pass first (rt_shadows reads the previous call's G-buffer: this camera's, whatever ran before), then the call"""
        self.set_params(**params)
        self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        self.gpu.render_hybrid(v, mask)

    def gathered(self, g, v, furnace=False):
        p = self.params
        key = (p["samples"], p["max_radiance"], furnace, int(v.total_samples), float(v.time), bytes(v.view))
        if key not in self._gathered:
            self._gathered[key] = (g,) + gi.gather(self.cpu, self.meshes, g, v, p, furnace)
        g0, counts, E, cast, totals, r = self._gathered[key]
        assert all(np.array_equal(bits(g0[k]), bits(g[k])) for k in ("position", "normal")), "the same G-buffer as the shared rays were made for"
        return counts, E, cast, totals, r

    def check(self, v, plain, furnace=False, sky=True):
        """the device's counts, totals, radiance and deferred output of the last render against the restatement on the device's G-buffer
        and ssao image; plain: deferred_output of the same calls without the bit (a twin context's). Everything exact is asserted here;
        sky: so is the tolerance on the pixels a missed ray enters (within_the_skys_tolerance)"""
        gpu, p = self.gpu, self.params
        g = gbuf(gpu)
        got_counts, got_rad, got_def, s = gpu.read_hybrid(COUNTS), gpu.read_hybrid(RADIANCE), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), gpu.rtgi_stats()
        counts, E, cast, totals, r = self.gathered(g, v, furnace)
        Ef, tainted = gi.filter(g, E, p, flag=counts[..., gi.MISSED] > 0)
        want_def, touched = gi.composite(g, gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), plain, Ef, v, self.meshes, p["intensity"])
        exact = ~tainted
        print(f"{p}: pixels {s.pixels} rays {s.rays} sun rays {s.shadow_rays} misses {s.misses} (want {totals}); differing counts "
              f"{(got_counts != counts).any(axis=-1).sum()}; radiance: {exact.sum()} pixels held bit for bit, {(bits(got_rad)[exact] != bits(Ef)[exact]).any(axis=-1).sum()} "
              f"differ; {tainted.sum()} within the sky's tolerance, max error {np.abs(got_rad[tainted] - Ef[tainted]).max() if tainted.any() else 0:.3e}; deferred: "
              f"{(bits(got_def)[exact] != bits(want_def)[exact]).any(axis=-1).sum()} of the exact pixels differ; trace {s.trace_ms:.3f} shadow {s.shadow_ms:.3f} "
              f"filter {s.filter_ms:.3f} composite {s.composite_ms:.3f} ms")
        assert got_counts.dtype == np.uint8 and got_counts.shape == (self.size[1], self.size[0], 4) and np.array_equal(got_counts, counts)
        assert integers(s) == totals and s.rays == s.pixels * p["samples"]
        assert s.trace_ms > 0 and s.shadow_ms > 0 and s.filter_ms > 0 and s.composite_ms > 0
        assert got_rad.dtype == np.float32 and np.array_equal(bits(got_rad)[exact], bits(Ef)[exact])
        assert np.array_equal(got_rad[..., 3] == 1, cast) and not got_rad[~cast].any()
        assert np.array_equal(bits(got_def)[exact], bits(want_def)[exact])
        got = dict(g=g, counts=got_counts, radiance=got_rad, deferred=got_def, cast=cast, exact=exact, touched=touched, want_radiance=Ef, want_deferred=want_def)
        if sky:
            within_the_skys_tolerance(got)
        return got


def within_the_skys_tolerance(got):
    """the pixels some tap of which has a missed ray: radiance and deferred output within what the sky pass's pixels are granted"""
    tainted = ~got["exact"]
    for name in ("radiance", "deferred"):
        a, b = got[name][tainted][:, :3], got["want_" + name][tainted][:, :3]
        err, bound = np.abs(a - b), SKY_ATOL + SKY_RTOL * np.abs(b)
        over = err > bound
        print(f"{name}: {over.sum()} of {over.size} channels of {tainted.sum()} pixels beyond rtol {SKY_RTOL} atol {SKY_ATOL}; largest error / bound "
              f"{(err / bound).max() if over.size else 0:.3f}" + (f" (got {a[over][0]:.8g}, want {b[over][0]:.8g})" if over.any() else ""))
    for name in ("radiance", "deferred"):
        assert np.allclose(got[name][tainted], got["want_" + name][tainted], rtol=SKY_RTOL, atol=SKY_ATOL), name


@pytest.fixture(scope="module")
def yard():
    return World(gi.courtyard_scene())


@pytest.fixture(scope="module")
def twin():
    """the courtyard on a context that never sets the bit: its deferred output is what the pass adds to"""
    return World(gi.courtyard_scene())


def plain_deferred(twin, v, mask=rr.HYBRID_FRAME):
    twin.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    twin.gpu.render_hybrid(v, mask)
    return twin.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)


# ---- 1. the device against the restatement ------------------------------------------------------------------------------------
_CASES = {}


def courtyard_case(yard, twin, samples, blur_radius, ssao):
    """one call on the courtyard with everything exact asserted (World.check), rendered once and shared by the two tests below"""
    key = (samples, blur_radius, ssao)
    if key not in _CASES:
        v = yard.view(ssao_enabled=ssao)
        yard.render(v, samples=samples, blur_radius=blur_radius)
        plain = plain_deferred(twin, v)
        _CASES[key] = dict(yard.check(v, plain, sky=False), plain=plain)
    return _CASES[key]


@pytest.mark.parametrize("ssao", [1, 0])
@pytest.mark.parametrize("blur_radius", [0, 1, 6])
@pytest.mark.parametrize("samples", [1, 3, 16])
def test_the_pass_equals_the_restatement(yard, twin, samples, blur_radius, ssao):
    got = courtyard_case(yard, twin, samples, blur_radius, ssao)
    cast, exact = got["cast"], got["exact"]
    assert cast.any() and not cast.all() and (exact & cast).any() and (~exact).any(), "pixels of both kinds"
    if samples > 1:  # (tests/test_rtgi_cpu.py proves these of the restatement at 3 and 16 samples; here on the device's G-buffer)
        assert blur_radius != 0 or (exact & cast).sum() >= 0.25 * cast.sum()
        assert ((got["counts"][..., gi.SUNLIT] > 0).sum() >= 0.1 * cast.sum()) and ((got["counts"][..., gi.MISSED] > 0).sum() >= 0.1 * cast.sum())
    plain = got["plain"]
    lit = got["touched"] & (got["radiance"][..., :3].sum(axis=-1) > 0)
    assert lit.any() and (got["deferred"][lit][:, :3] >= plain[lit][:, :3]).all() and (got["deferred"][lit][:, :3] > plain[lit][:, :3]).any()
    assert np.array_equal(bits(got["deferred"][~got["touched"]]), bits(plain[~got["touched"]])), "the sky and what did not cast are the plain frame's"
    assert np.array_equal(bits(got["deferred"][..., 3]), bits(plain[..., 3])), "alpha is untouched"


@pytest.mark.parametrize("ssao", [1, 0])
@pytest.mark.parametrize("blur_radius", [0, 1, 6])
@pytest.mark.parametrize("samples", [1, 3, 16])
def test_pixels_a_missed_ray_enters_are_within_the_skys_tolerance(yard, twin, samples, blur_radius, ssao):
    """UH_HYBRID_GI_RADIANCE and deferred_output on the pixels some counting tap of which has a missed ray, within rtol 1e-4, atol 1e-6 of
    the restatement: the tolerance hybrid_util.check_frame grants the sky pass's pixels.

    The courtyard's sample 0 of pixel (24, 19) leaves through the canopy's opening 5.8 degrees off the sun, where the Mie term carries
    the sky. With the hardware square root the other sky kernels take their heights with (1 ulp, and a height is a difference of
    float32 numbers near 6.4e6: half a metre per ulp, 4e-4 of the Mie density) the device gave 0.66508359 for its red channel against
    the oracle's 0.66500837: 1.114 times the bound, the one channel of 621 beyond it, and enough to miss at (samples, blur_radius) =
    (1, 0), (1, 1) and (3, 0). The pass's misses therefore take sky::integrate_scattering_exact_heights; measured on the MI355X the
    largest error is now 0.32 of the bound over all eighteen settings."""
    within_the_skys_tolerance(courtyard_case(yard, twin, samples, blur_radius, ssao))


@pytest.mark.parametrize("width, height", [(5, 3), (129, 2)])
def test_small_and_odd_frames(width, height):
    """fewer pixels than a wave, and two rows that end inside a fifth filter tile; the widest filter reaches beyond both"""
    w, t = World(gi.courtyard_scene(), width, height), World(gi.courtyard_scene(), width, height)
    v = w.view()
    w.render(v, samples=3, blur_radius=6)
    got = w.check(v, plain_deferred(t, v))
    assert got["cast"].any() and w.gpu.rtgi_stats().rays > 0


def test_both_layouts_of_the_trace_kernels_work_give_the_same_images(yard):
    v = yard.view()
    images, totals = [], []
    try:
        for order in (0, 1):
            yard.gpu.set_option("rtgi_order", order)
            yard.render(v, samples=3, blur_radius=1)
            images.append([yard.gpu.read_hybrid(i).view(np.uint8) for i in (COUNTS, RADIANCE, rr.HYBRID_DEFERRED_OUTPUT)])
            totals.append(integers(yard.gpu.rtgi_stats()))
    finally:
        yard.gpu.set_option("rtgi_order", 0)
    assert totals[0] == totals[1] and totals[0][0] > 0
    for a, b in zip(*images):
        assert np.array_equal(a, b)
    with pytest.raises(UtopianError, match="rtgi_order"):
        yard.gpu.set_option("rtgi_order", 2)


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples, blur_radius", [(1, 0), (3, 6), (16, 3)])
def test_a_bare_floor_under_the_furnace_receives_exactly_one(samples, blur_radius):
    w, t = World(gi.floor_scene()), World(gi.floor_scene())
    v = w.view()
    for x in (w, t):
        x.gpu.set_option("furnace", 1)
    w.render(v, samples=samples, blur_radius=blur_radius)
    got = w.check(v, plain_deferred(t, v), furnace=True)
    cast = got["cast"]
    assert cast.any() and not cast.all()
    assert (got["counts"][cast] == (0, 0, 0, samples)).all() and not got["counts"][~cast].any()
    assert (got["radiance"][cast] == 1.0).all() and not got["radiance"][~cast].any()
    s = w.gpu.rtgi_stats()
    assert integers(s) == (cast.sum(), samples * cast.sum(), 0, samples * cast.sum())


@pytest.mark.parametrize("samples, blur_radius", [(1, 0), (8, 6)])
def test_inside_a_closed_box_nothing_arrives(samples, blur_radius):
    w = World(gi.inward_box_scene())
    v = w.view()
    w.render(v, rr.HYBRID_FRAME, samples=samples, blur_radius=blur_radius)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v, samples=samples, blur_radius=blur_radius)
    got = w.check(v, plain)
    assert got["cast"].all() and (got["counts"] == (0, samples, 0, 0)).all()
    assert not got["radiance"][..., :3].any() and (got["radiance"][..., 3] == 1).all()
    assert np.array_equal(bits(got["deferred"]), bits(plain)), "the deferred output is the call's without the bit"
    s = w.gpu.rtgi_stats()
    assert s.pixels == W * H and s.rays == samples * W * H and s.misses == 0 and 0 < s.shadow_rays < s.rays


def test_an_emissive_wall_lights_the_wall_it_faces():
    w, t = World(gi.emissive_box_scene()), World(gi.emissive_box_scene())
    v = w.view()
    w.render(v, samples=16, blur_radius=0, max_radiance=0.5)
    got = w.check(v, plain_deferred(t, v))
    assert got["exact"].all(), "no ray misses: every pixel is held bit for bit"
    lit = got["counts"][..., gi.EMITTER] > 0
    assert lit.mean() > 0.5 and (got["radiance"][lit][:, :3] > 0).all() and (got["radiance"][..., :3] <= 0.5).all()
    assert not got["counts"][..., gi.SUNLIT].any() and not got["counts"][..., gi.MISSED].any()


def test_a_view_of_the_sky_alone_casts_nothing():
    scene = gi.floor_scene()
    scene.camera = rr.camera.Camera((0.0, 3.0, 6.0), (0.0, 30.0, 5.0), 60.0, W / H, 0.01, 1000.0)
    w, t = World(scene), World(scene)
    v = w.view()
    w.render(v, samples=3)  # the walks run on empty queues
    got = w.check(v, plain_deferred(t, v))
    assert not got["cast"].any() and not got["counts"].any() and not got["radiance"].any()
    assert integers(w.gpu.rtgi_stats()) == (0, 0, 0, 0)


# ---- 3. isolation -------------------------------------------------------------------------------------------------------------
def _path_tracer_state(r):
    s = r.get_stats()
    out = dict(acc=bits(r.read_accumulation()), out=r.read_output_bgra8(), pos=bits(r.read_gbuffer_position()),
               stats=np.array(list(s.rays) + [s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses], np.uint64))
    for k in range(3):
        out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
    return out


def _traced(frames):
    w = World(gi.courtyard_scene())
    w.loop = rr.FrameLoop(w.gpu, w.scene.make_view(W, H))
    for _ in range(frames):
        w.loop.frame(rr.PASS_ALL)
    return w


def test_the_bit_changes_nothing_but_the_deferred_output_and_its_own_images():
    a, b = _traced(3), _traced(3)
    v = a.view()
    rtao = rr.HYBRID_FRAME | rr.HYBRID_RTAO
    for x in (a, b):
        x.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        x.gpu.render_hybrid(v, rtao)
    before = _path_tracer_state(a.gpu)
    images_before, ao_before, ao_stats = read_all(a.gpu), a.gpu.read_hybrid(rr.HYBRID_AO_COUNTS), a.gpu.rtao_stats()
    a.gpu.set_rtgi_params(samples=3)
    a.gpu.render_hybrid(v, rtao | RTGI)
    after = _path_tracer_state(a.gpu)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    with_bit = read_all(a.gpu)
    for i in range(9):
        same = np.array_equal(images_before[i].view(np.uint8), with_bit[i].view(np.uint8))
        assert same == (i not in (rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_PRESENT_OUTPUT)), i
    s = a.gpu.rtao_stats()
    assert np.array_equal(a.gpu.read_hybrid(rr.HYBRID_AO_COUNTS), ao_before) and (s.pixels, s.rays, s.occluded) == (ao_stats.pixels, ao_stats.rays, ao_stats.occluded)
    assert a.gpu.rtgi_stats().rays > 0 and bytes(b.gpu.rtgi_stats()) == bytes(48)
    fa, fb = a.gpu.hybrid_frame_stats(), b.gpu.hybrid_frame_stats()
    assert (fa.sky_pixels, fa.lights) == (fb.sky_pixels, fb.lights) and all((x > 0) == (y > 0) for x, y in zip(fa.pass_ms, fb.pass_ms))
    # a frame without the bit on the same context: every image is the one of a context that never set it
    a.gpu.render_hybrid(v, rtao)
    b.gpu.render_hybrid(v, rtao)
    ia, ib = read_all(a.gpu), read_all(b.gpu)
    for i in range(9):
        assert np.array_equal(ia[i].view(np.uint8), ib[i].view(np.uint8)), i
        assert np.array_equal(ia[i].view(np.uint8), images_before[i].view(np.uint8)), i
    assert np.array_equal(a.gpu.read_hybrid(rr.HYBRID_AO_COUNTS), b.gpu.read_hybrid(rr.HYBRID_AO_COUNTS))
    # and the path tracer goes on as if the calls had not been made
    a.loop.frame(rr.PASS_ALL)
    b.loop.frame(rr.PASS_ALL)
    sa, sb = _path_tracer_state(a.gpu), _path_tracer_state(b.gpu)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    with pytest.raises(UtopianError, match="before the first rtgi pass"):
        b.gpu.read_hybrid(RADIANCE)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_fire_in_order_and_run_nothing(yard):
    gpu = yard.gpu
    v = yard.view()
    yard.render(v, samples=3, blur_radius=1)
    before = {**read_all(gpu), RADIANCE: gpu.read_hybrid(RADIANCE), COUNTS: gpu.read_hybrid(COUNTS)}
    stats_before = bytes(gpu.rtgi_stats())

    def unchanged(what):
        after = {**read_all(gpu), RADIANCE: gpu.read_hybrid(RADIANCE), COUNTS: gpu.read_hybrid(COUNTS)}
        for i in before:
            assert np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8)), (what, i)
        assert bytes(gpu.rtgi_stats()) == stats_before, what

    nan, inf = float("nan"), float("inf")
    bad = [("samples", 0), ("samples", 17), ("blur_radius", 7), ("max_radiance", 0.0), ("max_radiance", -1.0), ("max_radiance", nan), ("max_radiance", inf),
           ("intensity", -0.5), ("intensity", nan), ("intensity", inf), ("blur_normal_cos", nan), ("blur_plane", nan)]
    for field, value in bad:
        with pytest.raises(UtopianError, match=f"uh_set_rtgi_params: .*{field}") as e:
            gpu.set_rtgi_params(**gi.default_params(**{field: value}))
        assert "INVALID_ARGUMENT" in str(e.value)
        unchanged((field, value))
    # another camera: a call that ran would change every image. Each view breaks the rule under test and every rule behind it
    other = gi.courtyard_scene()
    other.camera = rr.camera.Camera((1.5, 1.2, 2.0), (0.0, 0.5, -2.0), 60.0, W / H, 0.01, 1000.0)
    fresh = World(gi.courtyard_scene())

    def moved(**kw):
        m = gi.scene_view(other, W, H)
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    no_deferred = rr.HYBRID_GBUFFER | RTGI
    cases = [(gpu, moved(raytracing_supported=0, ibl_enabled=1), RTGI, "UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(raytracing_supported=0, ibl_enabled=1), RTGI, "UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(ibl_enabled=1), RTGI, "UH_HYBRID_RTGI casts its rays from the G-buffer, and no G-buffer has been rendered"),
             (gpu, moved(ibl_enabled=1), no_deferred, "UH_HYBRID_RTGI with view.ibl_enabled = 1"),
             (gpu, moved(ibl_enabled=1), RTGI, "UH_HYBRID_RTGI with view.ibl_enabled = 1"),
             (gpu, moved(), no_deferred, "UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call"),
             (gpu, moved(), RTGI, "UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call")]
    for r, view, mask, message in cases:
        with pytest.raises(UtopianError, match=message) as e:
            r.render_hybrid(view, mask)
        assert "INVALID_ARGUMENT" in str(e.value)
        if r is gpu:
            unchanged(message)
        else:
            with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
                r.read_hybrid(rr.HYBRID_POSITION)
            assert bytes(r.rtgi_stats()) == bytes(48)
    # an existing rule comes first: the deferred pass with ibl_enabled = 1 and no IBL maps
    with pytest.raises(UtopianError, match="the deferred pass with view.ibl_enabled = 1 needs the IBL maps"):
        gpu.render_hybrid(moved(ibl_enabled=1, raytracing_supported=0), rr.HYBRID_GBUFFER | rr.HYBRID_DEFERRED | RTGI)
    unchanged("the deferred pass's rule")
    # the refused calls left the old params: the same view again gives the same images
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(v, FRAME)
    unchanged_but_times = {**read_all(gpu), RADIANCE: gpu.read_hybrid(RADIANCE), COUNTS: gpu.read_hybrid(COUNTS)}
    for i in before:
        assert np.array_equal(before[i].view(np.uint8), unchanged_but_times[i].view(np.uint8)), i
    # before the first pass: the images are refused and the stats are zero, with and without a frame
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
        fresh.gpu.read_hybrid(RADIANCE)
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    for which in (RADIANCE, COUNTS):
        with pytest.raises(UtopianError, match="images 18..19 before the first rtgi pass") as e:
            fresh.gpu.read_hybrid(which)
        assert "INVALID_ARGUMENT" in str(e.value)
    assert bytes(fresh.gpu.rtgi_stats()) == bytes(48)
    fresh.gpu.render_hybrid(v, rr.HYBRID_DEFERRED | RTGI)  # with a G-buffer from an earlier call it runs
    assert fresh.gpu.rtgi_stats().rays > 0 and fresh.gpu.read_hybrid(COUNTS).any()
    # before uh_build_acceleration, as without the bit
    empty = rr.Renderer(W, H)
    with pytest.raises(UtopianError, match="NOT_BUILT"):
        empty.render_hybrid(v, FRAME)


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------
def test_the_same_view_gives_the_same_bits_and_the_frame_number_seeds_the_rays(yard):
    gpu = yard.gpu
    v = yard.view()
    reads = lambda: [gpu.read_hybrid(i) for i in (COUNTS, RADIANCE, rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_PRESENT_OUTPUT)]
    yard.render(v, samples=3)
    first = reads()
    yard.render(v, samples=3)
    for a, b in zip(first, reads()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    later = yard.view(total_samples=v.total_samples + 1)
    yard.render(later, samples=3)
    second = reads()
    assert not np.array_equal(first[0], second[0]) and not np.array_equal(first[1], second[1])
    assert integers(gpu.rtgi_stats())[:2] == (first[1][..., 3].sum(), 3 * first[1][..., 3].sum())


# ---- 6. with TAA and the display chain ----------------------------------------------------------------------------------------
def test_taa_and_post_see_the_composited_frame(yard, twin):
    v = yard.view()
    chain = rr.HYBRID_TAA | rr.HYBRID_POST
    yard.gpu.reset_taa_history()
    yard.render(v, FRAME | chain, samples=3, blur_radius=1)
    plain = plain_deferred(twin, v)
    got = yard.check(v, plain)
    # the first taa pass has no history: its output is its input, the composited deferred output
    taa = yard.gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT)
    assert np.array_equal(bits(taa), bits(got["deferred"])) and not np.array_equal(bits(taa), bits(plain))
    assert (yard.gpu.read_hybrid(rr.HYBRID_TAA_HISTORY) == 1).all()
    s = yard.gpu.post_stats()
    assert s.renders >= 1 and s.tonemap_ms > 0 and yard.gpu.taa_stats().reset_pixels == W * H
    # and the pass sits before the sky pass: the sky pixels are the plain frame's
    sky = got["g"]["position"][..., 3] == 0
    assert sky.any() and np.array_equal(bits(got["deferred"][sky]), bits(plain[sky]))

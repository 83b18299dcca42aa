"""GPU: the ray-traced glossy reflections of the hybrid frame (uh_render_hybrid's UH_HYBRID_GLOSSY) against the restatement of
tests/glossy_reference.py on the device's own G-buffer, ssao image and the deferred output of a twin context without the bit: the ray
counts byte for byte with the pass's totals, the two images and the composited deferred output bit for bit wherever no missed ray enters
(and within the sky's tolerance where one does), the known answers, isolation, the refusals in their order, the frame behind RTGI's, frame
numbers that wrap and geometry that changed on the device."""
import numpy as np
import pytest

import glossy_reference as gl
import oracle_api as oa
import rust_renderer_amd as rr
from hybrid_util import bits, gbuf, pair, read_all
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

W, H = gl.W, gl.H
GLOSSY = rr.HYBRID_GLOSSY
SCALE, BIAS, COUNTS = rr.HYBRID_GLOSSY_SCALE, rr.HYBRID_GLOSSY_BIAS, rr.HYBRID_GLOSSY_COUNTS
OWN = (SCALE, BIAS, COUNTS)
FRAME = rr.HYBRID_FRAME | GLOSSY
# what hybrid_util.check_frame grants the sky pass's pixels of deferred_output: the device's IntegrateScattering against the oracle's
SKY_RTOL, SKY_ATOL = 1e-4, 1e-6
MEASURED = {}  # the largest error over its bound on the pixels a missed ray enters, by image (printed by the last test)


def integers(s):
    return (s.pixels, s.rays, s.below, s.shadow_rays, s.misses)


class World:
    """a scene on a GPU renderer and on the oracle; the restatement's rays of a view are computed once per setting on the device's
    G-buffer and shared by the checks that follow (the G-buffer is compared before they are reused)"""

    def __init__(self, scene, width=W, height=H):
        self.scene, self.size = scene, (width, height)
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        self._gathered = {}

    def set_oracle(self, cpu, meshes):
        self.cpu, self.meshes, self._gathered = cpu, meshes, {}

    def set_params(self, **params):
        self.params = gl.default_params(**params)
        self.gpu.set_glossy_params(**self.params)

    def view(self, **kw):
        return gl.scene_view(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        """a G-buffer pass first (rt_shadows reads the previous call's G-buffer: this camera's, whatever ran before), then the call"""
        self.set_params(**params)
        self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        self.gpu.render_hybrid(v, mask)

    def gathered(self, g, v, furnace=False):
        p = self.params
        key = (p["samples"], p["max_roughness"], p["max_radiance"], p["blur_roughness"], p["blur_radius"], furnace, int(v.total_samples), float(v.time), bytes(v.view))
        if key not in self._gathered:
            self._gathered[key] = (g, gl.gather(self.cpu, self.meshes, g, v, p, furnace))
        g0, got = self._gathered[key]
        assert all(np.array_equal(bits(g0[k]), bits(g[k])) for k in ("position", "normal", "pbr")), "the same G-buffer as the shared rays were made for"
        return got

    def check(self, v, plain, furnace=False):
        """the device's counts, totals, images and deferred output of the last render against the restatement on the device's G-buffer and
        ssao image; plain: deferred_output of the same calls without the bit (a twin context's). Exact where no counting tap has a
        missed ray, within the sky's tolerance elsewhere"""
        gpu, p = self.gpu, self.params
        g = gbuf(gpu)
        got_counts, got_s, got_b = gpu.read_hybrid(COUNTS), gpu.read_hybrid(SCALE), gpu.read_hybrid(BIAS)
        got_def, s = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), gpu.glossy_stats()
        want = self.gathered(g, v, furnace)
        Sf, Bf, info = gl.filter(g, want, p, flag=want["counts"][..., gl.MISSED] > 0)
        ssao = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE) if v.ssao_enabled == 1 else None
        want_def, touched = gl.composite(g, ssao, plain, Sf, Bf, v, self.meshes, p["intensity"])
        cast, exact = want["cast"], ~info["tainted"]
        print(f"{p}: {integers(s)} (want {want['totals']}); differing counts {(got_counts != want['counts']).any(axis=-1).sum()}; {exact.sum()} pixels held bit for "
              f"bit, {(~exact).sum()} within the sky's tolerance; trace {s.trace_ms:.3f} shade {s.shade_ms:.3f} shadow {s.shadow_ms:.3f} filter {s.filter_ms:.3f} "
              f"composite {s.composite_ms:.3f} ms")
        assert got_counts.dtype == np.uint8 and got_counts.shape == (self.size[1], self.size[0], 4) and np.array_equal(got_counts, want["counts"])
        assert integers(s) == want["totals"] and s.rays + s.below == s.pixels * p["samples"]
        assert s.trace_ms > 0 and s.shade_ms > 0 and s.shadow_ms > 0 and s.filter_ms > 0 and s.composite_ms > 0
        for name, a, b in (("scale", got_s, Sf), ("bias", got_b, Bf), ("deferred", got_def, want_def)):
            assert a.dtype == np.float32 and np.array_equal(bits(a)[exact], bits(b)[exact]), name
            x, y = a[~exact][:, :3], b[~exact][:, :3]
            bound = SKY_ATOL + SKY_RTOL * np.abs(y)
            worst = float((np.abs(x - y) / bound).max()) if x.size else 0.0
            MEASURED[name] = max(MEASURED.get(name, 0.0), worst)
            print(f"  {name}: largest error / bound on the other pixels {worst:.3f}")
            assert np.allclose(x, y, rtol=SKY_RTOL, atol=SKY_ATOL), name
        for img in (got_s, got_b):
            assert np.array_equal(img[..., 3] == 1, cast) and not img[~cast].any()
        assert np.array_equal(bits(got_def[..., 3]), bits(plain[..., 3])), "alpha is untouched"
        assert np.array_equal(bits(got_def[~touched]), bits(plain[~touched]))
        return dict(g=g, counts=got_counts, scale=got_s, bias=got_b, deferred=got_def, cast=cast, exact=exact, touched=touched, want=want)


def plain_deferred(twin, v, mask=rr.HYBRID_FRAME):
    twin.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    twin.gpu.render_hybrid(v, mask)
    return twin.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)


@pytest.fixture(scope="module")
def gallery():
    """the gallery at GALLERY_SIZE, the frame at which its adequacy is asserted (here on the device's G-buffer, in tests/test_glossy_cpu.py
    on the oracle's)"""
    return World(gl.gallery_scene(), *gl.GALLERY_SIZE)


@pytest.fixture(scope="module")
def twin():
    """the gallery on a context that never sets the bit: its deferred output is what the pass adds to"""
    return World(gl.gallery_scene(), *gl.GALLERY_SIZE)


# ---- 1. the device against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur_radius", [0, 1, 3, 6])
@pytest.mark.parametrize("samples", [1, 3, 16])
def test_the_pass_equals_the_restatement(gallery, twin, samples, blur_radius):
    v = gallery.view()
    gallery.render(v, samples=samples, blur_radius=blur_radius, blur_roughness=gl.GALLERY_BLUR_ROUGHNESS)
    plain = plain_deferred(twin, v)
    got = gallery.check(v, plain)
    cast, exact, want = got["cast"], got["exact"], got["want"]
    assert cast.any() and not cast.all() and (exact & cast).any() and (~exact).any(), "pixels of both kinds"
    # the fixture's adequacy on what the device rendered: the conditions of tests/test_glossy_cpu.py, on the device's own G-buffer
    px, p = want["px"], gallery.params
    kinds = [int(((want["kind"] == k) & ~want["below"]).sum()) for k in range(4)]
    _, _, info = gl.filter(got["g"], want, p, flag=want["counts"][..., gl.MISSED] > 0)
    clean = (exact & cast).sum() / cast.sum()
    print(f"kinds {kinds} below {want['below'].sum()} rough {px['rough'].sum()} metal {px['metal'].sum()} re == 0: {(px['re'] == 0).sum()} re == blur_radius: "
          f"{(px['re'] == blur_radius).sum()} dropped {info['dropped'].sum()} held bit for bit {clean:.3f}")
    if samples in (1, 16):
        assert min(kinds) >= 100 and want["below"].sum() >= 100, (kinds, want["below"].sum())
        assert px["rough"].sum() >= 100 and px["metal"].sum() >= 100
        assert (px["re"] == 0).sum() >= 100 and (px["re"] == blur_radius).sum() >= 100
        assert blur_radius < 3 or info["dropped"].sum() >= 100, "(at radius 1 the seams of the scene are 74 pixels long)"
        assert blur_radius > 3 or clean >= 0.2, "at the default radius and below, a fifth of the casting pixels is held bit for bit"
    lit = got["touched"] & ((got["scale"][..., :3].sum(axis=-1) + got["bias"][..., :3].sum(axis=-1)) > 0)
    assert lit.any() and (got["deferred"][lit][:, :3] >= plain[lit][:, :3]).all() and (got["deferred"][lit][:, :3] > plain[lit][:, :3]).any()


@pytest.mark.parametrize("width, height", [(5, 3), (129, 2)])
def test_small_and_odd_frames(width, height):
    """fewer pixels than a wave, and two rows that end inside a fifth filter tile; the widest filter reaches beyond both"""
    w, t = World(gl.gallery_scene(), width, height), World(gl.gallery_scene(), width, height)
    v = w.view()
    w.render(v, samples=3, blur_radius=6, blur_roughness=gl.GALLERY_BLUR_ROUGHNESS)
    got = w.check(v, plain_deferred(t, v))
    assert got["cast"].any() and w.gpu.glossy_stats().rays > 0


def test_ssao_off_and_rtgi_before_it(gallery, twin):
    """FRAME | RTGI | GLOSSY in one call: the restatement applied behind the rtgi pass's output (a twin's FRAME | RTGI); and with
    ssao_enabled = 0 the composite reads no ssao texel"""
    for kw, mask in ((dict(ssao_enabled=0), rr.HYBRID_FRAME), (dict(), rr.HYBRID_FRAME | rr.HYBRID_RTGI)):
        v = gallery.view(**kw)
        for x in (gallery, twin):
            x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        gallery.render(v, mask | GLOSSY, samples=3, blur_radius=3, blur_roughness=gl.GALLERY_BLUR_ROUGHNESS)
        plain = plain_deferred(twin, v, mask)
        got = gallery.check(v, plain)
        assert not np.array_equal(bits(got["deferred"]), bits(plain))
    assert gallery.gpu.rtgi_stats().rays > 0


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples, blur_radius", [(1, 0), (16, 3)])
def test_a_mirror_floor_under_the_furnace(samples, blur_radius):
    """r = 0 (tests/test_glossy_cpu.py): every ray is the mirror ray, misses and weighs exactly 1; at one sample per pixel the floor
    (metallic 1, base 1) receives exactly intensity * occlusion [* the ssao texel]"""
    w, t = World(gl.mirror_floor_scene()), World(gl.mirror_floor_scene())
    v = w.view(ssao_enabled=0)
    for x in (w, t):
        x.gpu.set_option("furnace", 1)
    w.render(v, samples=samples, blur_radius=blur_radius, intensity=0.75)
    plain = plain_deferred(t, v)
    got = w.check(v, plain, furnace=True)
    cast = got["cast"]
    assert cast.any() and not cast.all()
    assert (got["counts"][cast] == (0, 0, 0, samples)).all() and not got["counts"][~cast].any()
    s = w.gpu.glossy_stats()
    assert integers(s) == (cast.sum(), samples * cast.sum(), 0, 0, samples * cast.sum())
    total = got["scale"][cast][:, :3] + got["bias"][cast][:, :3]
    if samples == 1:
        assert (total == 1.0).all()
        added = got["deferred"][cast][:, :3] - plain[cast][:, :3]
        assert np.allclose(added, 0.75 * got["g"]["pbr"][cast][:, 2:3], rtol=1e-6, atol=1e-7)
    else:
        assert np.allclose(total, 1.0, rtol=1e-6)


@pytest.mark.parametrize("samples, blur_radius", [(1, 0), (8, 6)])
def test_inside_a_closed_box_nothing_arrives(samples, blur_radius):
    w = World(gl.inward_box_scene())
    v = w.view()
    w.render(v, rr.HYBRID_FRAME, samples=samples, blur_radius=blur_radius)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v, samples=samples, blur_radius=blur_radius)
    got = w.check(v, plain)
    assert got["cast"].all() and (got["counts"] == (0, samples, 0, 0)).all()
    for img in (got["scale"], got["bias"]):
        assert not img[..., :3].any() and (img[..., 3] == 1).all()
    assert np.array_equal(bits(got["deferred"]), bits(plain)), "the deferred output is the call's without the bit"
    s = w.gpu.glossy_stats()
    assert s.pixels == W * H and s.rays + s.below == samples * W * H and s.misses == 0 and 0 < s.shadow_rays < s.rays


def test_an_emissive_wall_is_mirrored_in_the_wall_it_faces():
    w, t = World(gl.emissive_box_scene()), World(gl.emissive_box_scene())
    v = w.view()
    w.render(v, samples=16, blur_radius=0, max_radiance=0.5)
    got = w.check(v, plain_deferred(t, v))
    assert got["exact"].all(), "no ray misses: every pixel is held bit for bit"
    want = got["want"]
    emit = want["kind"] == gl.EMITTER
    assert emit.sum() > 1000 and not got["counts"][..., gl.SUNLIT].any() and not got["counts"][..., gl.MISSED].any()
    total = (got["scale"][..., :3] + got["bias"][..., :3]).reshape(-1, 3)[want["px"]["rows"]]
    assert np.allclose(total, ((np.where(emit, want["Gw"], 0).astype(np.float64) * 0.5).sum(axis=1) / 16)[:, None], rtol=1e-5, atol=1e-7)


# ---- 3. isolation ---------------------------------------------------------------------------------------------------------------------
def test_with_the_bit_clear_everything_is_what_it_was(gallery, twin):
    """a context that has run the pass, then FRAME | RTGI without the bit: every image 0-19 and every counter equals a context that never set it"""
    v = gallery.view()
    gallery.render(v, FRAME | rr.HYBRID_RTGI, samples=3)
    own_before = [gallery.gpu.read_hybrid(i).copy() for i in OWN]
    stats_before = integers(gallery.gpu.glossy_stats())
    mask = rr.HYBRID_FRAME | rr.HYBRID_RTGI | rr.HYBRID_TAA
    for x in (gallery, twin):
        x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        x.gpu.reset_taa_history()
        x.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        x.gpu.render_hybrid(v, mask)
    for i in list(range(9)) + [rr.HYBRID_TAA_OUTPUT, rr.HYBRID_TAA_HISTORY, rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS]:
        assert np.array_equal(gallery.gpu.read_hybrid(i).view(np.uint8), twin.gpu.read_hybrid(i).view(np.uint8)), i
    a, b = gallery.gpu.rtgi_stats(), twin.gpu.rtgi_stats()
    assert (a.pixels, a.rays, a.shadow_rays, a.misses) == (b.pixels, b.rays, b.shadow_rays, b.misses)
    fa, fb = gallery.gpu.hybrid_frame_stats(), twin.gpu.hybrid_frame_stats()
    assert (fa.sky_pixels, fa.lights) == (fb.sky_pixels, fb.lights)
    sa, sb = gallery.gpu.hybrid_stats(), twin.gpu.hybrid_stats()
    assert list(sa.rays) == list(sb.rays) and sa.reflection_pixels == sb.reflection_pixels
    # the pass's own images and stats stay the last pass's; the twin never had them
    for i, before in zip(OWN, own_before):
        assert np.array_equal(gallery.gpu.read_hybrid(i).view(np.uint8), before.view(np.uint8))
    assert integers(gallery.gpu.glossy_stats()) == stats_before and bytes(twin.gpu.glossy_stats()) == bytes(64)
    for which in OWN:
        with pytest.raises(UtopianError, match="images 20..22 before the first glossy pass") as e:
            twin.gpu.read_hybrid(which)
        assert "INVALID_ARGUMENT" in str(e.value)


def test_with_the_bit_clear_every_image_of_every_pass_is_what_it_was():
    """images 0-19, the shadow maps and every counter, with every pass that makes one of them in the call (the scene, lights and
    reservoir frames of tests/test_gpu_hybrid_all_features.py, without the IBL maps and the display chain): a context whose first call
    carried the bit against one whose first call did not, on the second call of both, which carries no bit"""
    from test_gpu_hybrid_all_features import Context, counters, frame_views
    from test_gpu_rtgi_everything import ONE_CALL

    mask = ONE_CALL & ~rr.HYBRID_POST
    a, b = Context(), Context()
    v = frame_views(ibl=0)[0]
    a.gpu.set_glossy_params(samples=2, max_roughness=1.0)
    for x, first in ((a, mask | GLOSSY), (b, mask)):
        x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        x.begin(0, v)
        x.gpu.render_hybrid(v, first)
    assert a.gpu.glossy_stats().rays > 0 and bytes(b.gpu.glossy_stats()) == bytes(64)
    assert not np.array_equal(bits(a.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), bits(b.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT))), "the pass added something"
    own = [a.gpu.read_hybrid(i).copy() for i in OWN]
    for x in (a, b):
        x.gpu.reset_taa_history()
        x.gpu.render_hybrid(v, mask)
    for i in range(20):
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), b.gpu.read_hybrid(i).view(np.uint8)), i
    for c in range(4):
        assert np.array_equal(a.gpu.read_shadow_map(c).view(np.uint8), b.gpu.read_shadow_map(c).view(np.uint8)), c
    groups = ("shadow_maps", "shadows", "gbuffer", "motion", "reflections", "restir", "rtao", "deferred", "mc", "sky", "taa")
    assert counters(a.gpu, *groups) == counters(b.gpu, *groups)
    sa, sb = a.gpu.rtgi_stats(), b.gpu.rtgi_stats()
    assert (sa.pixels, sa.rays, sa.shadow_rays, sa.misses) == (sb.pixels, sb.rays, sb.shadow_rays, sb.misses) and sa.rays > 0
    for i, before in zip(OWN, own):
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), before.view(np.uint8)), "its own images stay the last pass's"


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_fire_in_order_and_run_nothing():
    gallery = World(gl.gallery_scene())
    gpu = gallery.gpu
    v = gallery.view()
    gallery.render(v, samples=3, blur_radius=1)
    snapshot = lambda: {**read_all(gpu), **{i: gpu.read_hybrid(i) for i in OWN}}
    before, stats_before = snapshot(), integers(gpu.glossy_stats())

    def unchanged(what):
        after = snapshot()
        for i in before:
            assert np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8)), (what, i)
        assert integers(gpu.glossy_stats()) == stats_before, what

    nan, inf = float("nan"), float("inf")
    bad = [("samples", 0), ("samples", 17), ("blur_radius", 7), ("max_roughness", -0.1), ("max_roughness", nan), ("max_roughness", inf), ("max_radiance", 0.0),
           ("max_radiance", nan), ("max_radiance", inf), ("intensity", -0.5), ("intensity", nan), ("intensity", inf), ("blur_roughness", 0.0),
           ("blur_roughness", nan), ("blur_roughness", inf), ("blur_normal_cos", nan), ("blur_plane", nan)]
    for field, value in bad:
        with pytest.raises(UtopianError, match=f"uh_set_glossy_params: .*{field}") as e:
            gpu.set_glossy_params(**gl.default_params(**{field: value}))
        assert "INVALID_ARGUMENT" in str(e.value)
        unchanged((field, value))
    # another camera: a call that ran would change every image. Each view breaks the rule under test and every rule behind it
    other = gl.gallery_scene()
    other.camera = rr.camera.Camera((1.5, 1.2, 2.0), (0.0, 0.5, -2.0), 60.0, W / H, 0.01, 1000.0)
    fresh = World(gl.gallery_scene())

    def moved(**kw):
        m = gl.scene_view(other, W, H)
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    no_deferred = rr.HYBRID_GBUFFER | GLOSSY
    cases = [(gpu, moved(raytracing_supported=0, ibl_enabled=1), GLOSSY, "UH_HYBRID_GLOSSY casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(raytracing_supported=0, ibl_enabled=1), GLOSSY, "UH_HYBRID_GLOSSY casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(ibl_enabled=1), GLOSSY, "UH_HYBRID_GLOSSY casts its rays from the G-buffer, and no G-buffer has been rendered"),
             (gpu, moved(ibl_enabled=1), no_deferred, "UH_HYBRID_GLOSSY with view.ibl_enabled = 1"),
             (gpu, moved(ibl_enabled=1), GLOSSY, "UH_HYBRID_GLOSSY with view.ibl_enabled = 1"),
             (gpu, moved(), no_deferred, "UH_HYBRID_GLOSSY without UH_HYBRID_DEFERRED in the same call"),
             (gpu, moved(), GLOSSY, "UH_HYBRID_GLOSSY without UH_HYBRID_DEFERRED in the same call"),
             # every existing rule first, RTGI's included
             (gpu, moved(raytracing_supported=0), rr.HYBRID_RTGI | GLOSSY, "UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1"),
             (gpu, moved(), rr.HYBRID_GBUFFER | rr.HYBRID_RTGI | GLOSSY, "UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call")]
    for r, view, mask, message in cases:
        with pytest.raises(UtopianError, match=message) as e:
            r.render_hybrid(view, mask)
        assert "INVALID_ARGUMENT" in str(e.value)
        if r is gpu:
            unchanged(message)
        else:
            with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
                r.read_hybrid(rr.HYBRID_POSITION)
            assert bytes(r.glossy_stats()) == bytes(64)
    # the refused calls left the old params: the same view again gives the same images
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(v, FRAME)
    again = snapshot()
    for i in before:
        assert np.array_equal(before[i].view(np.uint8), again[i].view(np.uint8)), i
    # before the first pass: the images are refused and the stats are zero, with and without a frame
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
        fresh.gpu.read_hybrid(SCALE)
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    for which in OWN:
        with pytest.raises(UtopianError, match="images 20..22 before the first glossy pass"):
            fresh.gpu.read_hybrid(which)
    assert bytes(fresh.gpu.glossy_stats()) == bytes(64)
    fresh.gpu.render_hybrid(v, rr.HYBRID_DEFERRED | GLOSSY)  # with a G-buffer from an earlier call it runs
    assert fresh.gpu.glossy_stats().rays > 0 and fresh.gpu.read_hybrid(COUNTS).any()
    # before uh_build_acceleration, as without the bit
    empty = rr.Renderer(W, H)
    with pytest.raises(UtopianError, match="NOT_BUILT"):
        empty.render_hybrid(v, FRAME)


# ---- 5. frame numbers and determinism -------------------------------------------------------------------------------------------------
def test_frame_numbers_that_wrap_in_32_bits(gallery, twin):
    """the seed word is (frame * 64 + s) ^ 0x474C4F53 in 32 bits. total_samples = 2^26 + 8: frame * 64 wraps to 512; time = -0.0001:
    frameNumber is 2^32 - 1 and frame * 64 = 0xFFFFFFC0. Both equal the restatement and differ from frame 0; the same view twice gives the same bits"""
    first = None
    for kw in (dict(), dict(), dict(total_samples=2 ** 26 + 8), dict(time=-0.0001)):
        v = gallery.view(**kw)
        frame = oa.frame_number(v)
        if kw:
            assert frame >= 2 ** 26 and (frame * 64) >= 2 ** 32
        gallery.render(v, samples=3, blur_radius=1)
        got = gallery.check(v, plain_deferred(twin, v))
        if first is None:
            assert frame == 0
            first = got
        elif not kw:
            for k in ("counts", "scale", "bias", "deferred"):
                assert np.array_equal(got[k].view(np.uint8), first[k].view(np.uint8)), k
        else:
            assert not np.array_equal(got["counts"], first["counts"]) and not np.array_equal(bits(got["scale"]), bits(first["scale"]))


# ---- 6. after the geometry changed on the device --------------------------------------------------------------------------------------
def _deform_frame(rs, w, t, v):
    w.render(v, samples=3, blur_radius=1, max_roughness=1.0)
    return w.check(v, plain_deferred(t, v))


def _changed_worlds(rs, scene):
    import test_gpu_mesh_deform as deform

    w, t = World(scene, deform.W, deform.H), World(scene, deform.W, deform.H)
    for x in (w, t):
        rs.on_the_oracle(x, scene)
    return w, t


def _assert_the_change_shows(w, v, got, before, stale):
    assert not np.array_equal(got["counts"], before["counts"]) and not np.array_equal(bits(got["scale"]), bits(before["scale"]))
    old = gl.gather(stale[0], stale[1], got["g"], v, w.params)
    assert not np.array_equal(old["counts"], got["counts"]) or not np.array_equal(bits(old["S"]), bits(got["want"]["S"])), "the restatement of the old geometry differs"


def test_after_update_mesh_vertices_with_a_refit():
    import test_gpu_mesh_deform as deform
    import test_gpu_rtgi_scenes as rs

    w, t = _changed_worlds(rs, rs.deform_scene(0))
    v = rs.deform_view(w)
    before = _deform_frame(rs, w, t, v)
    stale = (w.cpu, w.meshes)
    for x in (w, t):
        deform.update(x.gpu, deform.phase(2), "device")
        x.gpu.rebuild_tlas()
        rs.on_the_oracle(x, rs.deform_scene(2))
    got = _deform_frame(rs, w, t, v)
    assert got["want"]["totals"][1] > 0
    _assert_the_change_shows(w, v, got, before, stale)


def test_after_a_moved_instance_with_rebuild_tlas():
    import test_gpu_mesh_deform as deform
    import test_gpu_rtgi_scenes as rs

    w, t = _changed_worlds(rs, rs.deform_scene(0))
    before = _deform_frame(rs, w, t, rs.deform_view(w))
    stale = (w.cpu, w.meshes)
    for x in (w, t):
        x.gpu.set_instance_transform(deform.DEFORM, rs.MOVED_WORLD)
        rs.on_the_oracle(x, rs.deform_scene(0, deform_world=rs.MOVED_WORLD))
    v = rs.deform_view(w, rebuild_tlas=1)
    got = _deform_frame(rs, w, t, v)
    assert got["want"]["totals"][1] > 0
    _assert_the_change_shows(w, v, got, before, stale)


def test_report_the_largest_error_over_the_skys_bound():
    """not an assertion of its own (World.check asserts the bound per call): prints what DESIGN.md section 2 records"""
    print({k: round(x, 3) for k, x in MEASURED.items()})
    assert all(x <= 1.0 for x in MEASURED.values())

"""GPU: the ray-traced glass of the hybrid frame (uh_render_hybrid's UH_HYBRID_GLASS) against the restatement of tests/glass_reference.py
on the device's own G-buffer and the deferred output of a twin context without the bit: the counts image, the events image and every
statistic exactly, the radiance image and the composited deferred output bit for bit wherever no chain missed (and within the sky's
tolerance where one did), the known answers, the scene without glass, the refusals in their order, and isolation."""
import ctypes as C

import numpy as np
import pytest

import glass_reference as gs
import rust_renderer_amd as rr
from hybrid_util import bits, gbuf, pair, read_all
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

W, H = gs.W, gs.H
GLASS = rr.HYBRID_GLASS
RADIANCE, COUNTS, EVENTS = rr.HYBRID_GLASS_RADIANCE, rr.HYBRID_GLASS_COUNTS, rr.HYBRID_GLASS_EVENTS
OWN = (RADIANCE, COUNTS, EVENTS)
FRAME = rr.HYBRID_FRAME | GLASS
# what hybrid_util.check_frame grants the sky pass's pixels of deferred_output: the device's IntegrateScattering against the oracle's
SKY_RTOL, SKY_ATOL = 1e-4, 1e-6


class World:
    """a scene on a GPU renderer and on the oracle; the restatement's chains of a view are computed once per setting on the device's
    G-buffer and shared by the checks that follow (the G-buffer is compared before they are reused)"""

    def __init__(self, scene, width=W, height=H):
        self.scene, self.size = scene, (width, height)
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        self.ior = gs.iors(scene)
        self._chains = {}

    def view(self, **kw):
        return gs.scene_view(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        """a G-buffer pass first (rt_shadows reads the previous call's G-buffer: this camera's, whatever ran before), then the call"""
        self.params = gs.default_params(**params)
        self.gpu.set_glass_params(**self.params)
        self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        self.gpu.render_hybrid(v, mask)

    def chains(self, g, v, furnace=False, max_events=None):
        p = dict(self.params, max_events=self.params["max_events"] if max_events is None else max_events)
        key = (p["max_events"], p["max_radiance"], furnace, bytes(v.view))
        if key not in self._chains:
            self._chains[key] = (g, gs.chains(self.cpu, self.meshes, self.ior, g, v, p, furnace))
        g0, ch = self._chains[key]
        assert all(np.array_equal(bits(g0[k]), bits(g[k])) for k in ("position", "normal", "pbr")), "the same G-buffer as the shared chains were made for"
        return ch

    def check(self, v, plain, furnace=False):
        """the device's three images, stats and deferred output of the last render against the restatement on the device's G-buffer;
        plain: deferred_output of the same calls without the bit (a twin context's)"""
        gpu, p = self.gpu, self.params
        g = gbuf(gpu)
        got_rad, got_counts, got_ev = gpu.read_hybrid(RADIANCE), gpu.read_hybrid(COUNTS), gpu.read_hybrid(EVENTS)
        got_def, s = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), gpu.glass_stats()
        ch = self.chains(g, v, furnace)
        rad, counts, ev, cast, missed = gs.images(g, ch, p)
        want_def = gs.composite(plain, rad, p["intensity"])
        exact = ~missed
        print(f"{p} furnace {furnace}: {gs.integers(s)} (want {ch['totals']}); rounds {ch['rounds']}; differing counts "
              f"{(got_counts != counts).any(axis=-1).sum()} events {(got_ev != ev).any(axis=-1).sum()}; {(exact & cast).sum()} casting pixels held bit for bit, "
              f"{(~exact).sum()} within the sky's tolerance; trace {s.trace_ms:.3f} bend {s.bend_ms:.3f} shadow {s.shadow_ms:.3f} composite {s.composite_ms:.3f} ms")
        shape = (self.size[1], self.size[0], 4)
        assert got_counts.dtype == np.uint8 and got_counts.shape == shape and np.array_equal(got_counts, counts)
        assert got_ev.dtype == np.uint8 and got_ev.shape == shape and np.array_equal(got_ev, ev)
        assert gs.integers(s) == ch["totals"]
        assert s.chains + int(ch["tir0"].sum()) == 2 * s.pixels and s.segments == s.chains + s.events
        assert s.trace_ms > 0 and s.bend_ms > 0 and s.shadow_ms > 0 and s.composite_ms > 0
        for name, a, b in (("radiance", got_rad, rad), ("deferred", got_def, want_def)):
            assert a.dtype == np.float32 and a.shape == shape and np.array_equal(bits(a)[exact], bits(b)[exact]), name
            x, y = a[~exact][:, :3], b[~exact][:, :3]
            bound = SKY_ATOL + SKY_RTOL * np.abs(y)
            worst = float((np.abs(x - y) / bound).max()) if x.size else 0.0
            print(f"  {name}: largest error / bound on the pixels with a missed chain {worst:.3f} (DESIGN.md section 2 records the largest)")
            assert np.allclose(x, y, rtol=SKY_RTOL, atol=SKY_ATOL), name
        assert np.array_equal(got_rad[..., 3] == 1, cast) and not got_rad[~cast].any()
        assert np.array_equal(bits(got_def[..., 3]), bits(plain[..., 3])), "alpha is untouched"
        assert np.array_equal(bits(got_def[~cast]), bits(plain[~cast])), "no other pixel is touched"
        return dict(g=g, radiance=got_rad, counts=got_counts, events=got_ev, deferred=got_def, cast=cast, exact=exact, ch=ch)


def plain_deferred(twin, v, mask=rr.HYBRID_FRAME):
    twin.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    twin.gpu.render_hybrid(v, mask)
    return twin.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)


@pytest.fixture(scope="module")
def gallery():
    """the gallery at GALLERY_SIZE, the frame at which its adequacy is asserted (here on the device's G-buffer, in tests/test_glass_cpu.py
    on the oracle's)"""
    return World(gs.gallery_scene(), *gs.GALLERY_SIZE)


@pytest.fixture(scope="module")
def twin():
    """the gallery on a context that never sets the bit: its deferred output is what the pass replaces"""
    return World(gs.gallery_scene(), *gs.GALLERY_SIZE)


# ---- 1. the device against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("furnace", [0, 1])
@pytest.mark.parametrize("max_events", [1, 2, 8])
def test_the_pass_equals_the_restatement(gallery, twin, max_events, furnace):
    v = gallery.view()
    for x in (gallery, twin):
        x.gpu.set_option("furnace", furnace)
    try:
        gallery.render(v, max_events=max_events, intensity=0.75)
        plain = plain_deferred(twin, v)
        got = gallery.check(v, plain, furnace=bool(furnace))
    finally:
        for x in (gallery, twin):
            x.gpu.set_option("furnace", 0)
    cast, exact = got["cast"], got["exact"]
    assert cast.any() and not cast.all() and (exact & cast).any() and (~exact).any(), "pixels of both kinds"
    assert not np.array_equal(bits(got["deferred"][cast]), bits(plain[cast])), "the pass replaced what the deferred pass wrote"
    if max_events == 8 and not furnace:
        # the fixture's adequacy on what the device rendered: the conditions of tests/test_glass_cpu.py, on the device's own G-buffer
        print(gs.assert_adequate(got["ch"], gallery.chains(got["g"], v, max_events=2)))


@pytest.mark.parametrize("width, height", [(5, 3), (129, 2)])
def test_small_and_odd_frames(width, height):
    """fewer pixels than a wave, and two rows whose rays end inside a batch"""
    w, t = World(gs.gallery_scene(), width, height), World(gs.gallery_scene(), width, height)
    v = w.view()
    w.render(v, max_events=8)
    got = w.check(v, plain_deferred(t, v))
    assert got["cast"].any() and w.gpu.glass_stats().chains > 0


def test_behind_rtgi_and_glossy_the_pixel_is_still_replaced(gallery, twin):
    """FRAME | RTGI | GLOSSY | GLASS in one call: the restatement applied to a twin's FRAME | RTGI | GLOSSY - what those two added on a
    glass pixel is overwritten, what they added elsewhere stays"""
    mask = rr.HYBRID_FRAME | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY
    v = gallery.view()
    for x in (gallery, twin):
        x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        x.gpu.set_glossy_params(samples=1, blur_radius=1, max_roughness=1.0)
    gallery.render(v, mask | GLASS, max_events=8)
    plain = plain_deferred(twin, v, mask)
    got = gallery.check(v, plain)
    assert gallery.gpu.rtgi_stats().rays > 0 and gallery.gpu.glossy_stats().rays > 0
    assert not np.array_equal(bits(plain), bits(plain_deferred(twin, v))), "the two passes added something"


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------------
def test_with_one_event_the_ball_shows_its_reflection_alone(gallery, twin):
    """max_events = 1: chain 1 of the convex ball is cut, so C = R_0 exactly; on the ior-0.6 slab's TIR pixels C = clamp(L_0) and byte 1 is 0"""
    v = gallery.view()
    gallery.render(v, max_events=1)
    got = gallery.check(v, plain_deferred(twin, v))
    ch, rows = got["ch"], got["ch"]["px"]["rows"]
    mat = got["g"]["pbr"][..., 3].astype(np.uint32).reshape(-1)[rows]
    ball = (mat == gs.GALLERY_MESHES["ball"]) & ch["cut"][:, 1]
    held = got["exact"].reshape(-1)[rows]
    C, ev = got["radiance"].reshape(-1, 4)[rows][:, :3], got["events"].reshape(-1, 4)[rows]
    assert (ball & held).sum() >= 100 and np.array_equal(bits(C[ball & held]), bits(ch["R"][ball & held, 0]))
    assert (ev[ball, 2] & gs.CUT1).all() and (ev[ball, 1] == 1).all()
    tir = ch["tir0"] & (mat == gs.GALLERY_MESHES["thin"])
    assert tir.sum() >= 100 and (ev[tir, 1] == 0).all() and (ev[tir, 2] & gs.TIR).all() and (ch["weights"][tir, 0] == 1.0).all()
    assert (tir & held).any() and np.array_equal(bits(C[tir & held]), bits(ch["R"][tir & held, 0]))


@pytest.mark.parametrize("width, height", [(W, H)])
def test_nested_boxes(width, height):
    """the camera inside two glass boxes inside an emitter: every count is (0, 0, 2, 0), the events are the restatement's (3, 2), C is 1"""
    w = World(gs.nested_boxes_scene(), width, height)
    v = w.view()
    w.render(v, rr.HYBRID_FRAME)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v, max_events=8)
    got = w.check(v, plain)
    assert got["cast"].all() and got["exact"].all() and (got["counts"] == (0, 0, 2, 0)).all() and (got["events"] == (3, 2, 0, 0)).all()
    assert (np.abs(got["radiance"][..., :3].astype(np.float64) - 1.0) <= np.spacing(np.float32(1.0))).all()
    s = w.gpu.glass_stats()
    n = width * height
    assert gs.integers(s) == dict(pixels=n, chains=2 * n, segments=5 * n, events=3 * n, tir=0, cut=0, shadow_rays=0, misses=0)


def test_the_furnace_on_the_open_gallery(gallery, twin):
    """furnace, max_events = 16: a chain that ends on the sky or the lamp brings 1, one that ends on any other surface 0 (the rtgi pass's
    rule: dark under furnace). Where both chains bring 1 (or the one chain of a TIR pixel), C = w0 + w1 is within 1e-6 of 1"""
    v = gallery.view()
    for x in (gallery, twin):
        x.gpu.set_option("furnace", 1)
    try:
        gallery.render(v, max_events=16)
        got = gallery.check(v, plain_deferred(twin, v), furnace=True)
    finally:
        for x in (gallery, twin):
            x.gpu.set_option("furnace", 0)
    ch = got["ch"]
    bright = np.isin(ch["kind"], (gs.EMITTER, gs.MISSED))
    both = bright[:, 0] & (bright[:, 1] | ch["tir0"]) & ~ch["cut"].any(axis=1)
    C = got["radiance"].reshape(-1, 4)[ch["px"]["rows"]][:, :3]
    assert both.sum() >= 100 and (np.abs(C[both].astype(np.float64) - 1.0) <= 1e-6).all()
    assert gallery.gpu.glass_stats().shadow_rays == 0


# ---- 3. a scene without glass -------------------------------------------------------------------------------------------------------
def test_without_glass_the_pass_changes_nothing():
    """rtgi_reference's courtyard: the stats are zero apart from the times, the pass's images are zero, and every image the call
    makes, deferred_output among them, equals a call without the bit: 0..8, the rasterised G-buffer's 11..12, the rtao counts 14, the
    motion image 15 and 16..24. Images 9..10 need a marching-cubes field and 13 reservoir frames, which this scene has not; the isolation
    test below compares them on the all-features scene"""
    w, t = World(gs.no_glass_scene()), World(gs.no_glass_scene())
    v = w.view()
    mask = (rr.HYBRID_FRAME | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MOTION | rr.HYBRID_RTAO | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY | rr.HYBRID_FOG |
            rr.HYBRID_TAA)
    for x, m in ((w, mask | GLASS), (t, mask)):
        x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        x.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        x.gpu.render_hybrid(v, m)
    s = w.gpu.glass_stats()
    assert not any(gs.integers(s).values()) and s.trace_ms > 0 and s.bend_ms > 0 and s.shadow_ms > 0 and s.composite_ms > 0
    for i in OWN:
        assert not w.gpu.read_hybrid(i).any()
    for i in list(range(9)) + [11, 12, 14, 15] + list(range(16, 25)):
        assert np.array_equal(w.gpu.read_hybrid(i).view(np.uint8), t.gpu.read_hybrid(i).view(np.uint8)), i


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def raw_read(gpu, which):
    """uh_read_hybrid itself (Renderer.read_hybrid does not know images 25..27 before a call with the bit): the status and the message"""
    lib = rr.load_library()
    out = np.zeros((H, W, 4), np.float32)
    st = gpu._hybrid_api().read_hybrid(gpu._ctx, int(which), out.ctypes.data_as(C.c_void_p))
    lib.uh_last_error.restype, lib.uh_last_error.argtypes = C.c_char_p, [C.c_void_p]
    return st, lib.uh_last_error(gpu._ctx).decode()


def test_refusals_fire_in_order_and_run_nothing():
    gallery = World(gs.gallery_scene())
    gpu = gallery.gpu
    v = gallery.view()
    gallery.render(v, max_events=3)
    snapshot = lambda: {**read_all(gpu), **{i: gpu.read_hybrid(i) for i in OWN}}
    before, stats_before = snapshot(), gs.integers(gpu.glass_stats())

    def unchanged(what):
        after = snapshot()
        for i in before:
            assert np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8)), (what, i)
        assert gs.integers(gpu.glass_stats()) == stats_before, what

    for field, value in (("max_events", 0), ("max_events", 17), ("max_radiance", float("nan")), ("intensity", -1.0)):
        with pytest.raises(UtopianError, match=f"uh_set_glass_params: {field}") as e:
            gpu.set_glass_params(**gs.default_params(**{field: value}))
        assert "INVALID_ARGUMENT" in str(e.value)
        unchanged((field, value))
    # another camera: a call that ran would change every image. Each view breaks the rule under test and every rule behind it
    other = gs.gallery_scene()
    other.camera = rr.camera.Camera((1.5, 1.2, 2.0), (0.0, 0.5, -2.0), 60.0, W / H, 0.01, 1000.0)
    fresh = World(gs.gallery_scene())

    def moved(**kw):
        m = gs.scene_view(other, W, H)
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    no_deferred = rr.HYBRID_GBUFFER | GLASS
    cases = [(gpu, moved(raytracing_supported=0), GLASS, "UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(raytracing_supported=0), GLASS, "UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1"),
             (fresh.gpu, moved(), GLASS, "UH_HYBRID_GLASS casts its rays from the G-buffer, and no G-buffer has been rendered"),
             (gpu, moved(), no_deferred, "UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call"),
             (gpu, moved(), GLASS, "UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call"),
             # every earlier rule first: the glossy pass's and the fog pass's
             (gpu, moved(raytracing_supported=0), rr.HYBRID_GLOSSY | GLASS, "UH_HYBRID_GLOSSY casts rays and view.raytracing_supported is not 1"),
             (gpu, moved(), rr.HYBRID_GBUFFER | rr.HYBRID_FOG | GLASS, "UH_HYBRID_FOG without UH_HYBRID_DEFERRED and UH_HYBRID_SKY in the same call")]
    for r, view, mask, message in cases:
        with pytest.raises(UtopianError, match=message) as e:
            r.render_hybrid(view, mask)
        assert "INVALID_ARGUMENT" in str(e.value)
        if r is gpu:
            unchanged(message)
        else:
            with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
                r.read_hybrid(rr.HYBRID_POSITION)
            assert bytes(r.glass_stats()) == bytes(80)
    # the refused calls left the old params: the same view again gives the same images
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(v, FRAME)
    again = snapshot()
    for i in before:
        assert np.array_equal(before[i].view(np.uint8), again[i].view(np.uint8)), i
    # before the first pass: the Python layer does not know the images, the library refuses them, the stats are zero
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    for which in OWN:
        with pytest.raises(ValueError, match="0..15"):
            fresh.gpu.read_hybrid(which)
        st, message = raw_read(fresh.gpu, which)
        assert st == 1 and message == ("uh_read_hybrid: images 25..27 before the first glass pass (UH_HYBRID_GLASS); until then the image index must be 0..24")
    st, message = raw_read(fresh.gpu, 28)
    assert st == 1 and "image index must be 0..27" in message
    assert bytes(fresh.gpu.glass_stats()) == bytes(80)
    fresh.gpu.render_hybrid(v, rr.HYBRID_DEFERRED | GLASS)  # with a G-buffer from an earlier call it runs
    assert fresh.gpu.glass_stats().chains > 0 and fresh.gpu.read_hybrid(COUNTS).any()
    # before uh_build_acceleration, as without the bit
    empty = rr.Renderer(W, H)
    with pytest.raises(UtopianError, match="NOT_BUILT"):
        empty.render_hybrid(v, FRAME)


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------------------
def test_with_the_bit_clear_every_image_of_every_pass_is_what_it_was():
    """images 0-24, the shadow maps and every counter, with every pass that makes one of them (the scene, lights and reservoir frames of
    tests/test_gpu_hybrid_all_features.py, without the IBL maps and the display chain): a context whose first calls carried the bit
    against one whose first calls did not, on the second calls of both, which carry no bit. The fog pass refuses a call with the
    marching-cubes bit, so the all-features mask is two calls: one with the marching-cubes pass, then one with the fog pass, which runs
    behind the glass pass and reads the deferred_output it wrote. That scene has no glass: both contexts get a glass ball beside its
    metal sphere"""
    from rust_renderer_amd.scenes import icosphere
    from test_gpu_hybrid_all_features import Context, counters, frame_views
    from test_gpu_rtgi_everything import ONE_CALL

    with_mc = (ONE_CALL & ~rr.HYBRID_POST) | rr.HYBRID_GLOSSY
    with_fog = (with_mc & ~rr.HYBRID_MARCHING_CUBES) | rr.HYBRID_FOG
    assert with_fog & rr.HYBRID_SKY and with_fog & rr.HYBRID_DEFERRED
    a, b = Context(), Context()
    for x in (a, b):
        material = rr.make_material(rr.DIELECTRIC, 1.5, (1.0, 1.0, 1.0, 1.0), diffuse_map=x.gpu.default_diffuse_map())
        x.gpu.add_mesh(*icosphere(2), material, rr.transform3x4((7.0, 7.0, 7.0), (-4.0, 7.5, 0.0)))
        x.gpu.initialize_raytracing()
    v = frame_views(ibl=0)[0]
    a.gpu.set_glass_params(max_events=4)
    ran = []
    for x, bit in ((a, GLASS), (b, 0)):
        x.gpu.set_rtgi_params(samples=2, blur_radius=1)
        x.gpu.set_glossy_params(samples=2, max_roughness=1.0)
        x.begin(0, v)
        for mask in (with_mc, with_fog):
            x.gpu.render_hybrid(v, mask | bit)
            if bit:
                ran.append(gs.integers(x.gpu.glass_stats()))
    print(ran)
    assert all(r["pixels"] >= 100 and r["events"] > 0 for r in ran) and bytes(b.gpu.glass_stats()) == bytes(80)
    assert not np.array_equal(bits(a.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)), bits(b.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT))), "the pass replaced something"
    assert not np.array_equal(bits(a.gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT)), bits(b.gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT))), "and the fog and taa passes behind it saw that"
    own = [a.gpu.read_hybrid(i).copy() for i in OWN]
    for x in (a, b):
        x.gpu.reset_taa_history()
        for mask in (with_mc, with_fog):
            x.gpu.render_hybrid(v, mask)
    for i in range(25):
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), b.gpu.read_hybrid(i).view(np.uint8)), i
    for c in range(4):
        assert np.array_equal(a.gpu.read_shadow_map(c).view(np.uint8), b.gpu.read_shadow_map(c).view(np.uint8)), c
    groups = ("shadow_maps", "shadows", "gbuffer", "motion", "reflections", "restir", "rtao", "deferred", "mc", "sky", "taa")
    assert counters(a.gpu, *groups) == counters(b.gpu, *groups)
    sa, sb = a.gpu.rtgi_stats(), b.gpu.rtgi_stats()
    assert (sa.pixels, sa.rays, sa.shadow_rays, sa.misses) == (sb.pixels, sb.rays, sb.shadow_rays, sb.misses) and sa.rays > 0
    ga, gb = a.gpu.glossy_stats(), b.gpu.glossy_stats()
    assert (ga.pixels, ga.rays, ga.below, ga.shadow_rays, ga.misses) == (gb.pixels, gb.rays, gb.below, gb.shadow_rays, gb.misses) and ga.rays > 0
    fa, fb = a.gpu.fog_stats(), b.gpu.fog_stats()
    assert (fa.pixels, fa.rays, fa.lit) == (fb.pixels, fb.rays, fb.lit) and fa.rays > 0
    for i, before in zip(OWN, own):
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), before.view(np.uint8)), "its own images stay the last pass's"
    with pytest.raises(ValueError):
        b.gpu.read_hybrid(RADIANCE)

"""GPU: the volumetric fog pass of the hybrid frame (uh_render_hybrid's UH_HYBRID_FOG) against the restatement of tests/fog_reference.py on
the device's own G-buffer and deferred_output: the masks, the totals and every term but `a` bit for bit in each item layout; `a` within
2 ulp of numpy's exp, and with the device's own `a` fed back Ttot, F, Ff and deferred_output bit for bit; the slab scene's shafts against
the float64 predicate; the refusals in their order; frames of awkward sizes; the filter radii; the jitter; a camera from which no
geometry pixel marches; isolation from every other pass; and the taa pass behind it."""
import numpy as np
import pytest

import fog_reference as fog
import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao
import rust_renderer_amd as rr
import taa_reference as tr
from hybrid_util import bits, frame_view, gbuf, pair, synthetic_scene, ulps
from rust_renderer_amd.api import UtopianError

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

W, H = fog.W, fog.H
FOG = rr.HYBRID_FOG
FRAME = rr.HYBRID_FRAME | FOG
MASK, TERMS, DEFERRED = rr.HYBRID_FOG_MASK, rr.HYBRID_FOG_TERMS, rr.HYBRID_DEFERRED_OUTPUT


class World:
    """a scene on a GPU renderer and on the oracle; the restatement's masks of a view are computed once per (steps, march length, view)
    on the device's G-buffer and shared by the checks that follow (the G-buffer is compared before they are reused)"""

    def __init__(self, scene, width=W, height=H, view_of=frame_view, **fixed):
        self.scene, self.size, self.view_of, self.fixed = scene, (width, height), view_of, fixed
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        self._masks = {}

    def view(self, **kw):
        return self.view_of(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        """the frame without the bit, whose deferred_output is kept, then the frame with it (rt_shadows reads the previous call's
        G-buffer, so a G-buffer of this view goes first)"""
        self.params = fog.default_params(**{**self.fixed, **params})
        self.gpu.set_fog_params(**self.params)
        self.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        self.gpu.render_hybrid(v, mask & ~(FOG | rr.HYBRID_TAA | rr.HYBRID_POST))  # (the taa history advances once, in the call with the bit)
        self.plain = self.gpu.read_hybrid(DEFERRED)
        self.gpu.render_hybrid(v, mask)

    def want_masks(self, g, v, steps, max_distance):
        key = (steps, float(max_distance), int(v.total_samples), float(v.time), bytes(v.view), bytes(v.sun_dir))
        if key not in self._masks:
            self._masks[key] = (g,) + fog.masks(self.cpu, g["position"], v, steps, max_distance)
        g0, mask, totals = self._masks[key]
        assert np.array_equal(bits(g0["position"]), bits(g["position"])), "the same G-buffer as the shared masks were made for"
        return mask, totals

    def check(self, v):
        """the device's masks, totals, terms and deferred_output of the last render against the restatement"""
        gpu, p = self.gpu, self.params
        Ww, Hh = self.size
        g = gbuf(gpu)
        mask, terms, out, s = gpu.read_hybrid(MASK), gpu.read_hybrid(TERMS), gpu.read_hybrid(DEFERRED), gpu.fog_stats()
        want, (pixels, rays, lit) = self.want_masks(g, v, p["steps"], p["max_distance"])
        _, _, D, marched = fog.rays(g["position"], v, p["max_distance"])
        a_np = fog.attenuation(D, p["steps"], p["density"])
        a_dev = terms[..., 0].reshape(-1)
        a_ulp = ulps(a_dev[marched], a_np[marched]).max() if marched.any() else 0
        want_terms, want_out = fog.shade(want, g["position"], self.plain, v, p, a=a_dev)
        print(f"{p['steps']} steps, r {p['blur_radius']}: pixels {s.pixels} ({pixels}), rays {s.rays} ({rays}), lit {s.lit} ({lit}), differing masks "
              f"{(mask != want).sum()}, a within {a_ulp} ulp of numpy's, differing terms {(bits(terms[..., 1:]) != bits(want_terms[..., 1:])).sum()}, "
              f"differing texels {(bits(out) != bits(want_out)).sum()}; trace {s.trace_ms:.3f}, filter {s.filter_ms:.3f}, composite {s.composite_ms:.3f} ms")
        assert mask.dtype == np.uint32 and mask.shape == (Hh, Ww) and np.array_equal(mask, want)
        assert (s.pixels, s.rays, s.lit) == (pixels, rays, lit) and rays == pixels * p["steps"] and pixels == marched.sum()
        assert s.trace_ms > 0 and s.filter_ms > 0 and s.composite_ms > 0 and s.reserved == 0
        assert a_ulp <= 2 and not a_dev[~marched].any(), "OCML's expf and numpy's float32 exp are each documented to 1 ulp"
        assert np.array_equal(bits(terms[..., 1:]), bits(want_terms[..., 1:]))
        assert np.array_equal(bits(out), bits(want_out))
        return g, mask, terms, out


def slab_world(width=W, height=H):
    return World(fog.slab_scene(width, height), width, height, fog.slab_view, max_distance=fog.SLAB_MAX_DISTANCE, density=0.08)


@pytest.fixture(scope="module")
def floor():
    return World(fog.floor_scene(), density=0.05)


@pytest.fixture(scope="module")
def slab():
    return slab_world()


@pytest.fixture(scope="module")
def boxed():
    return World(ao.inward_box_scene(), density=0.3)


# ---- 1. the exact comparisons ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("steps", [1, 7, 32])
def test_masks_totals_terms_and_the_frame_equal_the_restatement(floor, slab, boxed, steps, order):
    """the bare floor (every bit set: with 32 steps bit 31), the slab (lit and dark samples along one ray) and the inside of the closed
    box (every mask 0), in each layout of the trace kernel's items"""
    full = np.uint32((1 << steps) - 1)
    for w in (floor, slab, boxed):
        v = w.view()
        w.gpu.set_option("fog_order", order)
        try:
            w.render(v, steps=steps)
            g, mask, terms, out = w.check(v)
        finally:
            w.gpu.set_option("fog_order", 2)
        marched = terms[..., 1] != 0
        if w is floor:
            assert (mask == full).all() and marched.all() and (steps < 32 or (mask >> 31).all())
            assert not np.array_equal(bits(out[..., :3]), bits(w.plain[..., :3])) and np.array_equal(bits(out[..., 3]), bits(w.plain[..., 3]))
        elif w is slab:
            assert (mask == 0).any() and (mask != 0).any() and (steps == 1 or ((mask != 0) & (mask != full)).any())
        else:
            assert (g["position"][..., 3] != 0).all() and not mask.any() and not terms[..., 2:].any() and marched.all()
            assert w.gpu.fog_stats().lit == 0 and w.gpu.fog_stats().pixels == W * H
    with pytest.raises(UtopianError, match="fog_order"):
        floor.gpu.set_option("fog_order", 3)


def test_counted_walks_leave_the_masks_and_fill_the_pass_s_own_counters(slab):
    gpu, v = slab.gpu, slab.view()
    before = gpu.get_stats()
    for order in (0, 1, 2):
        gpu.set_option("fog_order", order)
        try:
            slab.render(v, steps=7)
            mask = slab.check(v)[1]
            assert gpu.fog_visits() == (0, 0)
            gpu.set_option("count_visits", 1)
            slab.render(v, steps=7)
            gpu.set_option("count_visits", 0)
            assert np.array_equal(slab.check(v)[1], mask)
            nodes, tris = gpu.fog_visits()
            s = gpu.fog_stats()
            print(f"order {order}: {nodes / s.rays:.2f} node visits and {tris / s.rays:.2f} triangle tests per ray")
            assert nodes >= s.rays and tris >= s.rays - s.lit  # every ray visits the root; an occluded one tested its occluder
        finally:
            gpu.set_option("count_visits", 0)
            gpu.set_option("fog_order", 2)
    after = gpu.get_stats()
    assert list(after.rays) == list(before.rays) and after.closest_hits == before.closest_hits and after.misses == before.misses, "never UhStats"


# ---- 2. the shafts against geometry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [7, 32])
def test_the_slab_s_shafts_equal_the_float64_predicate(slab, steps):
    """the device's masks against the predicate of fog_reference.slab_predicate, with the exclusions test_fog_cpu.py holds to 2 %"""
    v = slab.view()
    slab.render(v, steps=steps, blur_radius=0)
    g, mask, _, _ = slab.check(v)
    rows, X = fog.sample_points(g["position"], v, steps, fog.SLAB_MAX_DISTANCE)
    lit, compared, inside = fog.slab_predicate(X, hr.sun_direction(v))
    got = ((mask.reshape(-1)[rows][:, None] >> np.arange(steps, dtype=np.uint32)[None, :]) & 1).astype(bool)
    print(f"steps {steps}: {1 - compared.mean():.4%} left out, {lit[compared].mean():.3f} lit, {(got != lit)[compared].sum()} disagree")
    assert inside.all() and 1 - compared.mean() <= 0.02 and lit[compared].mean() >= 0.10 and (~lit[compared]).mean() >= 0.10
    assert np.array_equal(got[compared], lit[compared])


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order_with_messages_and_nothing_run(floor):
    gpu = floor.gpu
    v = floor.view()
    floor.render(v, steps=7)
    _, mask_before, terms_before, out_before = floor.check(v)
    stats_before = (gpu.fog_stats().pixels, gpu.fog_stats().rays, gpu.fog_stats().lit, gpu.fog_stats().trace_ms)

    def unchanged(what):
        s = gpu.fog_stats()
        assert np.array_equal(gpu.read_hybrid(MASK), mask_before) and np.array_equal(bits(gpu.read_hybrid(TERMS)), bits(terms_before)), what
        assert np.array_equal(bits(gpu.read_hybrid(DEFERRED)), bits(out_before)) and (s.pixels, s.rays, s.lit, s.trace_ms) == stats_before, what

    other = fog.floor_scene()
    other.camera = rr.camera.Camera((1.0, 2.5, 5.0), (0.0, 0.0, 0.0), 60.0, W / H, 0.01, 1000.0)
    moved = frame_view(other, W, H)  # another camera: a call that ran would change every image
    fresh = World(fog.floor_scene())
    # each call breaks its own rule and every later one; the earlier rule is the one reported
    no_rt = frame_view(other, W, H)
    no_rt.raytracing_supported = 0
    with pytest.raises(UtopianError, match="UH_HYBRID_FOG casts sun rays and view.raytracing_supported is not 1") as e:
        fresh.gpu.render_hybrid(no_rt, FOG | rr.HYBRID_MARCHING_CUBES)
    assert "INVALID_ARGUMENT" in str(e.value)
    with pytest.raises(UtopianError, match="UH_HYBRID_FOG marches to the G-buffer's positions, and no G-buffer has been rendered"):
        fresh.gpu.render_hybrid(moved, FOG | rr.HYBRID_MARCHING_CUBES)
    for mask in (FOG, FOG | rr.HYBRID_DEFERRED, FOG | rr.HYBRID_SKY):
        with pytest.raises(UtopianError, match="UH_HYBRID_FOG without UH_HYBRID_DEFERRED and UH_HYBRID_SKY in the same call") as e:
            gpu.render_hybrid(moved, mask | rr.HYBRID_MARCHING_CUBES)
        assert "INVALID_ARGUMENT" in str(e.value)
        unchanged(mask)
    with pytest.raises(UtopianError, match="UH_HYBRID_FOG with UH_HYBRID_MARCHING_CUBES in the same call") as e:
        gpu.render_hybrid(moved, FRAME | rr.HYBRID_MARCHING_CUBES)
    assert "INVALID_ARGUMENT" in str(e.value)
    unchanged("marching cubes")
    with pytest.raises(UtopianError, match="UH_HYBRID_FOG casts sun rays"):
        gpu.render_hybrid(no_rt, FRAME)
    unchanged("raytracing_supported")
    # an earlier rule of another pass comes first
    with pytest.raises(UtopianError, match="UH_HYBRID_GBUFFER_RASTER without UH_HYBRID_GBUFFER"):
        gpu.render_hybrid(no_rt, FOG | rr.HYBRID_GBUFFER_RASTER)
    # read-back and stats before the first pass
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
        fresh.gpu.read_hybrid(MASK)
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    for image in (MASK, TERMS):
        with pytest.raises(UtopianError, match="images 23..24 before the first fog pass") as e:
            fresh.gpu.read_hybrid(image)
        assert "INVALID_ARGUMENT" in str(e.value)
    s = fresh.gpu.fog_stats()
    assert (s.pixels, s.rays, s.lit, s.trace_ms, s.filter_ms, s.composite_ms) == (0, 0, 0, 0.0, 0.0, 0.0) and fresh.gpu.fog_visits() == (0, 0)
    with pytest.raises(ValueError):
        fresh.gpu.read_hybrid(25)
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME & ~rr.HYBRID_GBUFFER | FOG)  # with a G-buffer from an earlier call it runs
    assert fresh.gpu.fog_stats().rays > 0 and fresh.gpu.read_hybrid(MASK).any()


# ---- 4. a view from which no geometry pixel marches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_geometry_pixel_whose_march_is_not_finite_keeps_its_colour(boxed, bad):
    """No verb writes the G-buffer and the cast leaves P = o + t d with t < 10000, so a position is never NaN or infinite; what the rule
    reads is V = P - o, and that is made non-finite here from the other side: the closed box's G-buffer from a good view, then a call
    without the G-buffer bit whose inverse_view puts the camera at NaN or infinity (eye_pos, which the deferred pass reads, stays). Every
    pixel is geometry, none marches: masks and terms 0, no ray cast, deferred_output exactly the frame's without the bit."""
    gpu = boxed.gpu
    v = boxed.view()
    gpu.set_fog_params(**fog.default_params(steps=7, density=0.3))
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    away = boxed.view()
    away.inverse_view[12] = bad
    rest = rr.HYBRID_FRAME & ~rr.HYBRID_GBUFFER
    gpu.render_hybrid(away, rest)
    plain = gpu.read_hybrid(DEFERRED)
    gpu.render_hybrid(away, rest | FOG)
    s = gpu.fog_stats()
    assert (gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0).all() and np.isfinite(plain).all()
    assert (s.pixels, s.rays, s.lit) == (0, 0, 0) and not gpu.read_hybrid(MASK).any() and not gpu.read_hybrid(TERMS).any()
    assert np.array_equal(bits(gpu.read_hybrid(DEFERRED)), bits(plain))
    _, _, D, marched = fog.rays(gpu.read_hybrid(rr.HYBRID_POSITION), away, 200.0)
    assert not marched.any() and not D.any(), "and the restatement agrees"
    # the good view again: every pixel marches
    boxed.render(v, steps=7)
    boxed.check(v)
    assert gpu.fog_stats().pixels == W * H


# ---- 5. frame sizes and the filter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", [(1, 1), (131, 3), (33, 9)])
def test_small_and_odd_frames(width, height):
    """one pixel; three rows that end inside a fifth filter tile; a width one past a tile and a height one past a tile row"""
    scene = fog.slab_scene(width, height)
    w = World(scene, width, height, fog.slab_view, max_distance=fog.SLAB_MAX_DISTANCE, density=0.08)
    v = w.view()
    for steps, blur_radius in ((7, 0), (32, 4)):
        w.render(v, steps=steps, blur_radius=blur_radius)
        w.check(v)
        assert w.gpu.fog_stats().pixels == width * height


@pytest.mark.parametrize("blur_radius", [0, 1, 4])
def test_the_filter_at_every_radius(slab, blur_radius):
    v = slab.view()
    slab.render(v, steps=7, blur_radius=blur_radius, blur_depth=0.1)
    g, _, terms, out = slab.check(v)
    if blur_radius == 0:
        assert np.array_equal(bits(terms[..., 2]), bits(terms[..., 3]))
    else:
        assert (terms[..., 2] != terms[..., 3]).any(), "the filter changes F"
        slab.render(v, steps=7, blur_radius=blur_radius, blur_depth=0.0)  # only taps at exactly the centre's march length count
        t0 = slab.check(v)[2]
        assert not np.array_equal(bits(t0[..., 3]), bits(terms[..., 3])), "the depth test stops taps"
    geo = g["position"][..., 3] != 0
    assert geo.any() and not geo.all(), "sky and geometry pixels both filter"


# ---- 6. the jitter ---------------------------------------------------------------------------------------------------------------------
def test_a_moved_sun_and_a_second_frame_number_give_new_masks(slab):
    v = slab.view()
    slab.render(v, steps=7)
    first = slab.check(v)[1]
    slab.render(v, steps=7)
    assert np.array_equal(slab.check(v)[1], first), "the same view: the same xi"
    later = slab.view(total_samples=v.total_samples + 1)
    slab.render(later, steps=7)
    second = slab.check(later)[1]
    assert not np.array_equal(first, second), "a new frame number: a new xi"
    rows = np.arange(W * H)
    assert not np.array_equal(fog._jitter(W, H, oa.frame_number(v))[rows], fog._jitter(W, H, oa.frame_number(later))[rows])
    moved = slab.view()
    moved.sun_dir[:] = (-0.3, 1.0, 0.1)
    slab.render(moved, steps=7)
    third = slab.check(moved)[1]
    assert not np.array_equal(first, third), "the shaft moves with the sun"


# ---- 7. isolation ------------------------------------------------------------------------------------------------------------------------
def _integers(r):
    s, a, g, l = r.get_stats(), r.rtao_stats(), r.rtgi_stats(), r.glossy_stats()
    return dict(stats=list(s.rays) + [s.frames, s.closest_hits, s.misses], rtao=(a.pixels, a.rays, a.occluded),
                rtgi=(g.pixels, g.rays, g.shadow_rays, g.misses), glossy=(l.pixels, l.rays, l.below, l.shadow_rays, l.misses))


def test_the_bit_changes_nothing_but_the_frame_and_its_own_images():
    """two contexts fed identically, one frame with every ray pass and the bit, one without it: every hybrid image but deferred_output
    and present, and every other pass's integers, agree bit for bit; and a frame without the bit after one with it is the plain frame"""
    scene = synthetic_scene()
    a, b = World(scene), World(scene)
    v = a.view()
    every = rr.HYBRID_FRAME | rr.HYBRID_RTAO | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY
    for w, mask in ((a, every | FOG), (b, every)):
        w.gpu.set_fog_params(**fog.default_params(steps=7))
        w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        w.gpu.render_hybrid(v, mask)
    images = [i for i in list(range(9)) + [rr.HYBRID_AO_COUNTS] + list(range(18, 23)) if i not in (DEFERRED, rr.HYBRID_PRESENT_OUTPUT)]
    for i in images:
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), b.gpu.read_hybrid(i).view(np.uint8)), i
    assert _integers(a.gpu) == _integers(b.gpu)
    assert not np.array_equal(bits(a.gpu.read_hybrid(DEFERRED)), bits(b.gpu.read_hybrid(DEFERRED))) and a.gpu.fog_stats().rays > 0
    with pytest.raises(UtopianError, match="images 23..24 before the first fog pass"):
        b.gpu.read_hybrid(MASK)
    own = [a.gpu.read_hybrid(i).copy() for i in (MASK, TERMS)]
    stats = (a.gpu.fog_stats().pixels, a.gpu.fog_stats().lit, a.gpu.fog_stats().trace_ms)
    for w in (a, b):
        w.gpu.render_hybrid(v, every)
    for i in list(range(9)) + [rr.HYBRID_AO_COUNTS] + list(range(18, 23)):
        assert np.array_equal(a.gpu.read_hybrid(i).view(np.uint8), b.gpu.read_hybrid(i).view(np.uint8)), i
    assert all(np.array_equal(x.view(np.uint8), a.gpu.read_hybrid(i).view(np.uint8)) for x, i in zip(own, (MASK, TERMS))), "its images stay"
    assert (a.gpu.fog_stats().pixels, a.gpu.fog_stats().lit, a.gpu.fog_stats().trace_ms) == stats


def test_the_taa_pass_integrates_the_fogged_frame(slab):
    """UH_HYBRID_TAA and UH_HYBRID_POST in the same call, two frame numbers from a resting camera: taa_output is taa_reference fed the
    restatement's fogged frames"""
    gpu = slab.gpu
    ref, params = tr.Taa(), tr.default_params()
    gpu.set_taa_params(**params)
    gpu.reset_taa_history()
    blended = 0
    for call in range(2):
        v = slab.view(total_samples=3 + call)
        pv = (np.array(v.projection[:], np.float32).reshape(4, 4).T @ np.array(v.view[:], np.float32).reshape(4, 4).T).T.reshape(-1)
        v.prev_frame_projection_view[:] = pv.tolist()
        slab.render(v, FRAME | rr.HYBRID_TAA | rr.HYBRID_POST, steps=7)
        g, mask, terms, out = slab.check(v)
        want_terms, fogged = fog.shade(mask, g["position"], slab.plain, v, slab.params, a=terms[..., 0].reshape(-1))
        want = ref(fogged, g["position"], None, v, params, W, H)
        assert np.array_equal(bits(gpu.read_hybrid(rr.HYBRID_TAA_OUTPUT)), bits(want["output"])), call
        blended = int(want["blended"].sum())
    assert blended > W * H // 2, "the second call blends the first's fogged frame"
    gpu.reset_taa_history()

"""GPU: ray-traced ambient occlusion in the hybrid frame's SSAO slot (uh_render_hybrid's UH_HYBRID_RTAO) against the restatement of
tests/rtao_reference.py on the device's own G-buffer: the occluded-ray counts byte for byte with the pass's totals, ssao_output exactly
with and without the filter, known answers (a bare floor, the inside of a closed box, the sky alone), the radius, the deferred output,
edge shapes, the gates, the refusals, isolation from the path tracer and stream order."""
import numpy as np
import pytest

import hybrid_frame_reference as fr
import rtao_reference as ao
import rust_renderer_amd as rr
from hybrid_util import DEFERRED_ULP, bits, frame_view, gbuf, pair, read_all, synthetic_scene, ulps
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

W, H = ao.W, ao.H
RTAO = rr.HYBRID_RTAO
COUNTS = rr.HYBRID_AO_COUNTS
FRAME = rr.HYBRID_FRAME | RTAO


def stats_tuple(s):
    return (s.pixels, s.rays, s.occluded, s.trace_ms, s.filter_ms)


class World:
    """a scene on a GPU renderer and on the oracle; the restatement's counts of a view are computed once per (samples, radius, frame
    number) on the device's G-buffer and shared by the checks that follow (the G-buffer is compared before they are reused)"""

    def __init__(self, scene, width=W, height=H):
        self.scene, self.size = scene, (width, height)
        self.gpu, self.cpu, self.meshes = pair(scene, width, height)
        self._counts = {}

    def view(self, **kw):
        return frame_view(self.scene, *self.size, **kw)

    def render(self, v, mask=FRAME, **params):
        self.params = ao.default_params(**params)
        self.gpu.set_rtao_params(**self.params)
        self.gpu.render_hybrid(v, mask)

    def want_counts(self, g, v, samples, radius):
        key = (samples, float(radius), int(v.total_samples), float(v.time), bytes(v.view))
        if key not in self._counts:
            self._counts[key] = (g,) + ao.counts(self.cpu, g, v, samples, radius)
        g0, count, totals = self._counts[key]
        assert all(np.array_equal(bits(g0[k]), bits(g[k])) for k in ("position", "normal")), "the same G-buffer as the shared counts were made for"
        return count, totals

    def check(self, v):
        """the device's counts, totals and ssao_output of the last render against the restatement on the device's G-buffer"""
        gpu, p = self.gpu, self.params
        g = gbuf(gpu)
        count, img, s = gpu.read_hybrid(COUNTS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), gpu.rtao_stats()
        want, (pixels, rays, occluded) = self.want_counts(g, v, p["samples"], p["radius"])
        want_img = ao.resolve(g, want, p["samples"], p["strength"], p["blur_radius"], p["blur_normal_cos"], p["blur_plane"])
        print(f"{p}: pixels {s.pixels} ({pixels}), rays {s.rays} ({rays}), occluded {s.occluded} ({occluded}), differing counts {(count != want).sum()}, "
              f"differing texels {(img != want_img).sum()}, trace {s.trace_ms:.3f} ms, filter {s.filter_ms:.3f} ms")
        assert count.dtype == np.uint8 and count.shape == (self.size[1], self.size[0]) and np.array_equal(count, want)
        assert (s.pixels, s.rays, s.occluded) == (pixels, rays, occluded) and rays == pixels * p["samples"]
        assert s.trace_ms > 0 and s.filter_ms > 0
        assert img.dtype == np.uint16 and np.array_equal(img, want_img)
        return g, count, img


@pytest.fixture(scope="module")
def synthetic():
    return World(synthetic_scene())


@pytest.fixture(scope="module")
def boxed():
    return World(ao.inward_box_scene())


# ---- 1. the counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 8, 64])
def test_counts_equal_the_restatement_byte_for_byte(synthetic, boxed, samples):
    """the synthetic scene, then the inside of the closed box: between them a count of 0 and a count of `samples` both occur at every
    sample count (in the synthetic scene alone the largest count at 64 samples is 58: some ray of every pixel reaches the sky)"""
    seen = set()
    for w, radius in ((synthetic, 1.0), (boxed, ao.BOX_RADIUS)):
        v = w.view()
        w.render(v, samples=samples, radius=radius)
        _, count, _ = w.check(v)
        seen |= set(np.unique(count).tolist())
    assert min(seen) == 0 and max(seen) == samples


# ---- 2. the image -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [1.0, 1.6])
@pytest.mark.parametrize("blur_radius", [0, 1, 2, 4])
def test_ssao_output_equals_the_restatement_exactly(synthetic, blur_radius, strength):
    v = synthetic.view()
    synthetic.render(v, samples=8, strength=strength, blur_radius=blur_radius)
    g, count, img = synthetic.check(v)
    cast = ao.normals(g)[1].reshape(H, W)
    assert (img[::-1][~cast] == 65535).all() and cast.any() and not cast.all()
    if strength == 1.6 and blur_radius == 0:
        assert (count == 8).any() and (img[::-1][count >= 5] == 0).all(), "1 - 1.6 * 5 / 8 and below clamp at 0"
    if blur_radius:
        synthetic.render(v, samples=8, strength=strength, blur_radius=0)
        assert not np.array_equal(synthetic.gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), img), "the filter changes the image"


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------
def test_a_bare_floor_is_unoccluded():
    w = World(ao.floor_scene())
    v = w.view()
    w.render(v, samples=8, radius=4.0, strength=1.6)
    g, count, img = w.check(v)
    geo = g["position"][..., 3] != 0
    assert geo.any() and not geo.all() and not count.any() and (img == 65535).all()
    s = w.gpu.rtao_stats()
    assert (s.pixels, s.rays, s.occluded) == (geo.sum(), 8 * geo.sum(), 0)


@pytest.mark.parametrize("strength, blur_radius", [(1.0, 0), (0.25, 2), (1.6, 4)])
def test_inside_a_closed_box_every_ray_is_occluded(boxed, strength, blur_radius):
    v = boxed.view()
    boxed.render(v, samples=8, radius=ao.BOX_RADIUS, strength=strength, blur_radius=blur_radius)
    g, count, img = boxed.check(v)
    assert (g["position"][..., 3] != 0).all() and (count == 8).all()
    assert (img == int(fr.unorm16(np.float32(1.0) - np.float32(strength)))).all()
    s = boxed.gpu.rtao_stats()
    assert s.pixels == W * H and s.occluded == s.rays == 8 * W * H


def test_a_view_of_the_sky_alone_casts_nothing():
    scene = synthetic_scene()
    scene.camera = rr.camera.Camera((0.0, 2.2, 6.5), (0.0, 30.0, 5.0), 60.0, W / H, 0.01, 1000.0)
    w = World(scene)
    v = w.view()
    w.render(v, samples=8)  # the trace kernel runs on an empty queue
    g, count, img = w.check(v)
    assert not (g["position"][..., 3] != 0).any() and not count.any() and (img == 65535).all()
    assert stats_tuple(w.gpu.rtao_stats())[:3] == (0, 0, 0)


# ---- 4. the radius ------------------------------------------------------------------------------------------------------------
def test_counts_grow_with_the_radius(synthetic):
    v = synthetic.view()
    got = []
    for radius in (0.25, 1.0, 4.0):
        synthetic.render(v, samples=8, radius=radius)
        got.append(synthetic.check(v)[1])
    a, b, c = got
    assert (a <= b).all() and (b <= c).all() and a.sum() < b.sum() < c.sum()


@pytest.mark.parametrize("order", [0, 1, 2])
def test_every_layout_of_the_trace_kernels_work_gives_the_same_counts(synthetic, order):
    """option "rtao_order": one ray per item with a pixel's samples together, one ray per item with one sample of consecutive pixels
    together, one pixel per item; 3 samples do not divide a wave, 64 is the cap. With "count_visits" the walks are counted, and the
    counts stay"""
    gpu = synthetic.gpu
    v = synthetic.view()
    gpu.set_option("rtao_order", order)
    try:
        for samples in (3, 64):
            synthetic.render(v, samples=samples, radius=4.0)
            _, count, _ = synthetic.check(v)
            assert gpu.rtao_visits() == (0, 0)
            gpu.set_option("count_visits", 1)
            synthetic.render(v, samples=samples, radius=4.0)
            gpu.set_option("count_visits", 0)
            assert np.array_equal(synthetic.check(v)[1], count)
            nodes, tris = gpu.rtao_visits()
            rays = gpu.rtao_stats().rays
            print(f"order {order}, {samples} samples: {nodes / rays:.2f} node visits and {tris / rays:.2f} triangle tests per ray")
            assert nodes >= rays and tris >= gpu.rtao_stats().occluded  # every ray visits the root; an occluded one tested its occluder
    finally:
        gpu.set_option("count_visits", 0)
        gpu.set_option("rtao_order", 0)
    with pytest.raises(UtopianError, match="rtao_order"):
        gpu.set_option("rtao_order", 3)


# ---- 5. the deferred output ---------------------------------------------------------------------------------------------------
def test_deferred_output_multiplies_by_the_rtao_image(synthetic):
    gpu = synthetic.gpu
    v = synthetic.view()
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)  # rt_shadows reads the previous call's G-buffer: this camera's
    synthetic.render(v, samples=8)
    g, _, img = synthetic.check(v)
    d = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    ref = fr.deferred(g, gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), img, v, synthetic.meshes, [])
    geo = g["position"][..., 3] != 0
    u = ulps(d[geo], ref[geo])
    print(f"deferred: max {u.max()} ulp, exact on {(u == 0).mean():.4f} of the geometry pixels' channels")
    assert geo.any() and np.isfinite(d[geo]).all() and u.max() <= DEFERRED_ULP
    assert gpu.hybrid_frame_stats().pass_ms[3] == 0.0, "ssao.frag's kernel is not launched"
    synthetic.render(synthetic.view(ssao_enabled=0), samples=8)
    plain = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    assert (d[geo][:, :3] <= plain[geo][:, :3]).all() and (d[geo][:, :3] < plain[geo][:, :3]).any()
    assert np.array_equal(bits(d[~geo]), bits(plain[~geo])), "the sky does not change"


# ---- 6. edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", [(5, 3), (64, 1), (129, 2)])
def test_small_and_odd_frames(width, height):
    """fewer pixels than a wave, one row of exactly a wave, and two rows that end inside a fifth filter tile"""
    scene = synthetic_scene()
    if width > 8 * height:  # a strip: a narrow lens from the same place, or nearly every ray leaves the scene sideways
        scene.camera = rr.camera.Camera((0.0, 2.2, 6.5), (0.0, 0.5, 0.0), 1.2, width / height, 0.01, 1000.0)
    w = World(scene, width, height)
    v = w.view()
    for samples, blur_radius in ((3, 0), (8, 4)):
        w.render(v, samples=samples, radius=4.0, blur_radius=blur_radius)
        g, _, _ = w.check(v)
        assert (g["position"][..., 3] != 0).any() and w.gpu.rtao_stats().rays > 0


# ---- 7. the gates -------------------------------------------------------------------------------------------------------------
def test_without_ssao_enabled_the_pass_does_not_run(synthetic):
    gpu = synthetic.gpu
    v = synthetic.view()
    synthetic.render(v, samples=3)
    before, counts_before, stats_before = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), gpu.read_hybrid(COUNTS), stats_tuple(gpu.rtao_stats())
    off = synthetic.view(ssao_enabled=0, total_samples=v.total_samples + 5)
    for mask in (FRAME, FRAME & ~rr.HYBRID_SSAO):
        synthetic.render(off, mask, samples=8)
        assert np.array_equal(gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), before) and np.array_equal(gpu.read_hybrid(COUNTS), counts_before)
        assert stats_tuple(gpu.rtao_stats()) == stats_before
    # with it, the pass runs whether or not the SSAO bit is set, and ssao.frag's kernel does not
    synthetic.render(v, RTAO, samples=3)
    assert np.array_equal(gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), before) and gpu.hybrid_frame_stats().pass_ms[3] == 0.0
    synthetic.check(v)


def test_without_the_bit_the_frame_is_the_plain_one(synthetic):
    v = synthetic.view()
    synthetic.render(v, samples=8, strength=1.6)
    synthetic.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    plain = World(synthetic.scene)
    for _ in range(2):  # (rt_shadows reads the previous call's G-buffer)
        plain.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    a, b = read_all(synthetic.gpu), read_all(plain.gpu)
    for i in range(9):
        assert np.array_equal(a[i].view(np.uint8), b[i].view(np.uint8)), i
    assert np.array_equal(a[rr.HYBRID_SSAO_IMAGE], fr.ssao(a[rr.HYBRID_POSITION], a[rr.HYBRID_NORMAL], v)), "ssao.frag's image again"
    assert synthetic.gpu.hybrid_frame_stats().pass_ms[3] > 0.0


def test_the_frame_number_seeds_the_rays(synthetic):
    gpu = synthetic.gpu
    v = synthetic.view()
    synthetic.render(v, samples=8)
    _, first, img = synthetic.check(v)
    synthetic.render(v, samples=8)
    assert np.array_equal(gpu.read_hybrid(COUNTS), first) and np.array_equal(gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), img)
    later = synthetic.view(total_samples=v.total_samples + 1)
    synthetic.render(later, samples=8)
    _, second, _ = synthetic.check(later)
    assert not np.array_equal(first, second)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_run_nothing(synthetic):
    gpu = synthetic.gpu
    v = synthetic.view()
    synthetic.render(v, samples=3, radius=2.0)
    _, counts_before, _ = synthetic.check(v)
    before, stats_before = read_all(gpu), stats_tuple(gpu.rtao_stats())

    def unchanged(what):
        after = read_all(gpu)
        for i in range(9):
            assert np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8)), (what, i)
        assert np.array_equal(gpu.read_hybrid(COUNTS), counts_before) and stats_tuple(gpu.rtao_stats()) == stats_before, what

    nan, inf = float("nan"), float("inf")
    bad = [("samples", 0), ("samples", 65), ("radius", 0.0), ("radius", -1.0), ("radius", nan), ("radius", inf), ("radius", 20000.0),
           ("strength", nan), ("strength", -0.5), ("blur_radius", 5)]
    for field, value in bad:
        with pytest.raises(UtopianError, match=f"uh_set_rtao_params: {field}") as e:
            gpu.set_rtao_params(**ao.default_params(**{field: value}))
        assert "INVALID_ARGUMENT" in str(e.value)
        unchanged((field, value))
    other = synthetic_scene()
    other.camera = rr.camera.Camera((1.0, 1.5, 5.0), (0.0, 0.5, 0.0), 60.0, W / H, 0.01, 1000.0)
    moved = frame_view(other, W, H)  # another camera: a call that ran would change every image
    moved.raytracing_supported = 0
    with pytest.raises(UtopianError, match="UH_HYBRID_RTAO casts occlusion rays and view.raytracing_supported") as e:
        gpu.render_hybrid(moved, FRAME)
    assert "INVALID_ARGUMENT" in str(e.value)
    unchanged("raytracing_supported")
    # the refused calls left the old params: the same view again gives the same counts
    gpu.render_hybrid(v, FRAME)
    assert np.array_equal(gpu.read_hybrid(COUNTS), counts_before) and stats_tuple(gpu.rtao_stats())[:3] == stats_before[:3]
    # a context without a G-buffer, and the counts before the first pass
    fresh = World(synthetic.scene)
    with pytest.raises(UtopianError, match="no G-buffer has been rendered"):
        fresh.gpu.render_hybrid(v, RTAO)
    with pytest.raises(UtopianError, match="before the first uh_render_hybrid"):
        fresh.gpu.read_hybrid(rr.HYBRID_POSITION)
    assert stats_tuple(fresh.gpu.rtao_stats()) == (0, 0, 0, 0.0, 0.0)
    fresh.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    fresh.gpu.render_hybrid(synthetic.view(ssao_enabled=0), FRAME)  # the bit without ssao_enabled: no pass yet
    with pytest.raises(UtopianError, match="image 14"):
        fresh.gpu.read_hybrid(COUNTS)
    assert stats_tuple(fresh.gpu.rtao_stats()) == (0, 0, 0, 0.0, 0.0)
    fresh.gpu.render_hybrid(v, RTAO)  # and with a G-buffer from an earlier call it runs
    assert fresh.gpu.rtao_stats().rays > 0 and fresh.gpu.read_hybrid(COUNTS).any()


# ---- 9. isolation and stream order --------------------------------------------------------------------------------------------
def _path_tracer_state(r):
    s = r.get_stats()
    out = dict(acc=bits(r.read_accumulation()), out=r.read_output_bgra8(), pos=bits(r.read_gbuffer_position()),
               stats=np.array(list(s.rays) + [s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses], np.uint64))
    for k in range(3):
        out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
    return out


def _traced(scene, frames):
    w = World(scene)
    w.loop = rr.FrameLoop(w.gpu, scene.make_view(W, H))
    for _ in range(frames):
        w.loop.frame(rr.PASS_ALL)
    return w


def test_a_call_with_the_bit_changes_nothing_the_path_tracer_reads():
    scene = synthetic_scene()
    a, b = _traced(scene, 3), _traced(scene, 3)
    v = a.view()
    before = _path_tracer_state(a.gpu)
    a.render(v, samples=8)
    after = _path_tracer_state(a.gpu)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert a.gpu.rtao_stats().rays > 0
    # the path tracer goes on as if the call had not been made
    a.loop.frame(rr.PASS_ALL)
    b.gpu.render_hybrid(v, rr.HYBRID_FRAME)
    b.loop.frame(rr.PASS_ALL)
    sa, sb = _path_tracer_state(a.gpu), _path_tracer_state(b.gpu)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_frames_in_flight_then_the_hybrid_call_equal_the_serial_sequence():
    scene = synthetic_scene()

    def run(serial):
        w = _traced(scene, 0)
        v = w.view()
        w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
        for _ in range(4):
            w.loop.frame(rr.PASS_ALL)
            if serial:
                w.gpu.synchronize()
        w.render(v, samples=8)            # no wait in between
        w.loop.frame(rr.PASS_ALL)         # and a frame behind it
        if serial:
            w.gpu.synchronize()
        s = w.gpu.rtao_stats()
        return dict(counts=w.gpu.read_hybrid(COUNTS), ssao=w.gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), deferred=bits(w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)),
                    totals=np.array([s.pixels, s.rays, s.occluded]), **_path_tracer_state(w.gpu))

    a, b = run(False), run(True)
    assert a["totals"][2] > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k

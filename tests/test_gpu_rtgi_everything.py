"""GPU: the rtgi pass among its neighbours. The scene, lights, moves and views of test_gpu_hybrid_all_features.py without the IBL maps (the
rtgi pass refuses view.ibl_enabled = 1), over three frames on three contexts. Context A renders each frame as one call with FRAME |
SHADOW_MAPS | GBUFFER_RASTER | MOTION | RESTIR_LIGHTS | RTAO | RTGI | MARCHING_CUBES | TAA | POST; context B renders it as separate calls
in the pass order of hybrid_passes (csrc/hybrid_graph.hip); context C follows B up to the deferred pass without the RTGI bit, so its
deferred output is what B's rtgi pass added to. On B the rtgi pass is held to the restatement of tests/rtgi_reference.py on B's
rasterised G-buffer, the ssao image its rtao call made and C's reservoir-lit, shadow-mapped deferred output (test_gpu_rtgi.World.check);
the other passes are held by test_gpu_hybrid_all_features.py. After every frame every readable image and every counter of A equals B's.

What hybrid_plan couples within a call, and B therefore keeps together: RESTIR_LIGHTS | DEFERRED | RTGI (the rtgi pass is refused
without the deferred pass in its call, and the deferred pass reads the visibility image only with RESTIR_LIGHTS in its call),
MARCHING_CUBES | SKY, and TAA | POST | PRESENT (the post pass reads taa_output, and present post_output, only within one call)."""
import numpy as np
import pytest

import hybrid_reference as hr
import oracle_api as oa
import rtgi_reference as gi
import rust_renderer_amd as rr
from hybrid_util import bits
from test_gpu_hybrid_all_features import FRAMES, MOVED, MOVES, Context, H, W, counters, frame_views, scene_at
from test_gpu_rtgi import World, integers

pytestmark = pytest.mark.gpu

RTGI = rr.HYBRID_RTGI
ONE_CALL = (rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MOTION | rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_RTAO | RTGI |
            rr.HYBRID_MARCHING_CUBES | rr.HYBRID_TAA | rr.HYBRID_POST)
LIT = rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_DEFERRED
# B's calls with the counter groups each one produces (the stats structs describe the last call that ran their pass)
BEFORE_THE_PASS = [(rr.HYBRID_SHADOW_MAPS, ("shadow_maps",)), (rr.HYBRID_RT_SHADOWS, ("shadows",)),
                   (rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MOTION, ("gbuffer", "motion")), (rr.HYBRID_RT_REFLECTIONS, ("reflections",)),
                   (rr.HYBRID_RTAO, ("rtao",))]
THE_PASS = (LIT | RTGI, ("restir", "deferred", "rtgi"))
AFTER_THE_PASS = [(rr.HYBRID_MARCHING_CUBES | rr.HYBRID_SKY, ("mc", "sky")), (rr.HYBRID_TAA | rr.HYBRID_POST | rr.HYBRID_PRESENT, ("taa", "post"))]
CALLS = BEFORE_THE_PASS + [THE_PASS] + AFTER_THE_PASS
assert sum(m for m, _ in CALLS) == ONE_CALL & ~rr.HYBRID_SSAO, "the separate calls are the one call's bits (the rtao pass takes ssao's place)"
PARAMS = dict(samples=2, blur_radius=1)
GROUPS = tuple(name for _, names in CALLS for name in names)  # (no env: no IBL maps)


def images(gpu):
    """every image of the frame: read_hybrid's 0..19, the shadow maps and the display chain's"""
    out = {i: gpu.read_hybrid(i) for i in range(20)}
    out.update({f"shadow map {c}": gpu.read_shadow_map(c) for c in range(4)})
    out.update(post=gpu.read_post(rr.POST_OUTPUT), histogram=gpu.read_post(rr.POST_HISTOGRAM))
    for k in range(1, gpu.post_stats().levels + 1):
        out.update({f"bloom down {k}": gpu.read_post(rr.POST_BLOOM_DOWN, k), f"bloom up {k}": gpu.read_post(rr.POST_BLOOM_UP, k)})
    return out


def some_counters(gpu, which=GROUPS):
    """test_gpu_hybrid_all_features.counters, with the rtgi pass's and the display chain's (its exposure as bits)"""
    own = dict(rtgi=lambda: integers(gpu.rtgi_stats()),
               post=lambda: (lambda p: (bits(np.float32([p.exposure, p.target_exposure, p.average_luminance])).tolist(), p.metered_pixels, p.bad_pixels, p.levels,
                                        p.renders))(gpu.post_stats()))
    out = counters(gpu, *[n for n in which if n not in own])
    out.update({n: own[n]() for n in which if n in own})
    return out


@pytest.fixture(scope="module")
def contexts():
    a, b, c = Context(), Context(), Context()
    for x in (a, c):
        x.gpu.set_rtgi_params(**PARAMS)
    cpu = oa.OracleRenderer(W, H)
    hr.upload_recorded(scene_at(0), cpu, False)
    for l in a.lights:
        cpu.add_gpu_light(l)
    cpu.initialize_raytracing()
    return a, b, c, cpu


def restated(b, cpu):
    """context B and the oracle as a test_gpu_rtgi.World, whose check is the restatement on the device's own inputs"""
    w = World(None, W, H, on=(b.gpu, cpu, b.meshes))
    w.set_params(**PARAMS)
    return w


def test_the_rtgi_pass_in_one_call_with_everything_equals_the_passes_one_at_a_time(contexts):
    a, b, c, cpu = contexts
    w = restated(b, cpu)
    seen = {}
    for k, v in enumerate(frame_views(ibl=0)):
        assert (v.ibl_enabled, v.cubemap_enabled, v.shadows_enabled, v.ssao_enabled, v.raytracing_supported) == (0, 0, 1, 1, 1)
        for x in (a, b, c):
            x.begin(k, v)
        if k:
            cpu.set_instance_transform(MOVED, MOVES[k])
            cpu.initialize_raytracing()
        a.gpu.render_hybrid(v, ONE_CALL)
        want_count = {}
        for mask, names in BEFORE_THE_PASS:
            b.gpu.render_hybrid(v, mask)
            want_count.update(some_counters(b.gpu, names))
            c.gpu.render_hybrid(v, mask)
        c.gpu.render_hybrid(v, LIT)
        plain = c.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        b.gpu.render_hybrid(v, THE_PASS[0])
        want_count.update(some_counters(b.gpu, THE_PASS[1]))
        for i in (rr.HYBRID_POSITION, rr.HYBRID_NORMAL, rr.HYBRID_PBR, rr.HYBRID_SSAO_IMAGE, rr.HYBRID_LIGHT_VISIBILITY, rr.HYBRID_SHADOWS):
            assert np.array_equal(b.gpu.read_hybrid(i).view(np.uint8), c.gpu.read_hybrid(i).view(np.uint8)), f"frame {k}: B's and C's input {i} of the deferred pass"
        w.forget()  # (the key does not know the moved instance)
        got = w.check(v, plain)
        assert b.gpu.gbuffer_raster_stats().renders == k + 1 and b.gpu.rtao_stats().rays > 0, "a rasterised G-buffer, an ssao image the rtao pass made"
        lit = got["touched"] & (got["radiance"][..., :3].sum(axis=-1) > 0)
        assert lit.sum() >= 100 and (got["deferred"][lit][:, :3] >= plain[lit][:, :3]).all() and (got["deferred"][lit][:, :3] > plain[lit][:, :3]).any()
        assert np.array_equal(bits(got["deferred"][~got["touched"]]), bits(plain[~got["touched"]]))
        r = w.gathered(got["g"], v)[4]
        for mask, names in AFTER_THE_PASS:
            b.gpu.render_hybrid(v, mask)
            want_count.update(some_counters(b.gpu, names))
        got_images, want_images = images(a.gpu), images(b.gpu)
        assert got_images.keys() == want_images.keys()
        for name in want_images:
            assert np.array_equal(got_images[name].view(np.uint8), want_images[name].view(np.uint8)), f"frame {k}: image {name} of the one call differs from the separate calls'"
        got_count = some_counters(a.gpu)
        assert got_count == want_count, f"frame {k}: {[(n, got_count[n], want_count[n]) for n in want_count if got_count[n] != want_count[n]]}"
        covered = b.gpu.read_hybrid(rr.HYBRID_MARCHING_CUBES_VISIBILITY) != rr.MARCHING_CUBES_NONE
        seen = dict(on_the_moved_box=int((r["mesh"] == MOVED).sum()), iso_over_gi=int((covered & lit).sum()), taa=want_count["taa"], rtgi=want_count["rtgi"],
                    sunlit=int((got["counts"][..., gi.SUNLIT] > 0).sum()), missed=int((got["counts"][..., gi.MISSED] > 0).sum()), exact=int((got["exact"] & got["cast"]).sum()))
        print(f"frame {k + 1}: {seen}")
    assert k + 1 == FRAMES
    assert seen["on_the_moved_box"] >= 10, "rays of the rtgi pass meet the box where it stands in frame three"
    assert seen["iso_over_gi"] > 0, "the marching-cubes pass draws over pixels that received GI"
    assert seen["taa"][0] > 0, "the taa pass has history"
    assert seen["sunlit"] > 0 and seen["missed"] > 0 and seen["exact"] > 0 and seen["rtgi"][2] > 0

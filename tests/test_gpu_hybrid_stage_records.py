"""GPU: which timed-stage records a call resets, runs and keeps - uh_render_hybrid, uh_render_forward and uh_denoise over call
sequences on the synthetic scene at 24 x 16, read back through every stats verb. A record is 0.0 exactly when its stage did not run
in the call that last reset it, above 0 when it ran, and a record a call leaves alone reads the same bits afterwards."""
import pytest

import rust_renderer_amd as rr
from hybrid_util import add_lights, frame_view, synthetic_scene
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

W, H = 24, 16
SHADOWS, GBUFFER, REFLECTIONS, SSAO, DEFERRED, SKY, PRESENT = range(7)  # pass_ms of UhHybridFrameStats, bit order
ENV, MAPS, MC, RESTIR, RTAO, MOTION = (rr.HYBRID_ENVIRONMENT, rr.HYBRID_SHADOW_MAPS, rr.HYBRID_MARCHING_CUBES, rr.HYBRID_RESTIR_LIGHTS,
                                       rr.HYBRID_RTAO, rr.HYBRID_MOTION)


class World:
    """the synthetic scene with two lights on a renderer, the cascades set (64 x 64 maps) and one reservoir frame rendered"""

    def __init__(self):
        self.scene = synthetic_scene()
        self.gpu = self.scene.upload(rr.Renderer(W, H))
        add_lights(self.gpu, 2, seed=5)
        self.gpu.set_option("shadow_map_size", 64)
        self.gpu.set_shadowmap_params(rr.shadow_cascades(self.scene.camera, self.view().sun_dir[:]))
        rr.FrameLoop(self.gpu, self.scene.make_view(W, H)).frame(rr.PASS_RESTIR)

    def view(self, **kw):
        v = frame_view(self.scene, W, H)
        v.num_lights = 2
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def records(self):
        """every stage record and render count the stats verbs report, by name"""
        g = self.gpu
        out = {f"frame{k}": ms for k, ms in enumerate(g.hybrid_frame_stats().pass_ms)}
        out.update({f"hybrid{k}": ms for k, ms in enumerate(g.hybrid_stats().pass_ms)})  # G-buffer, rt_shadows, rt_reflections
        e, sm, mc, gr = g.environment_stats(), g.shadow_map_stats(), g.marching_cubes_stats(), g.gbuffer_raster_stats()
        out.update({f"env{k}": ms for k, ms in enumerate(e.pass_ms)})
        out.update(env_builds=e.builds, maps=sm.pass_ms, maps_renders=sm.renders, mc=mc.pass_ms, mc_renders=mc.renders, raster=gr.pass_ms,
                   raster_renders=gr.renders, restir=g.hybrid_restir_stats().pass_ms)
        ao, mv, fw = g.rtao_stats(), g.motion_stats(), g.forward_stats()
        out.update(rtao_trace=ao.trace_ms, rtao_filter=ao.filter_ms, motion=mv.motion_ms, snapshot=mv.snapshot_ms, forward_renders=fw.renders)
        out.update({f"forward{k}": ms for k, ms in enumerate(fw.pass_ms)})
        out.update({f"denoise{k}": ms for k, ms in enumerate(g.denoise_stats().pass_ms)})
        return out


@pytest.fixture
def world():
    return World()


def frame_passes(rec):
    """the seven pass records: the indices above 0; the others are 0.0 exactly"""
    ms = [rec[f"frame{k}"] for k in range(7)]
    assert all(m == 0.0 or m > 0.0 for m in ms)
    assert [rec["hybrid0"], rec["hybrid1"], rec["hybrid2"]] == [ms[GBUFFER], ms[SHADOWS], ms[REFLECTIONS]], "both verbs read the same records"
    return {k for k in range(7) if ms[k] > 0.0}


def env_passes(rec):
    ms = [rec[f"env{k}"] for k in range(4)]
    assert all(m == 0.0 or m > 0.0 for m in ms)
    return {k for k in range(4) if ms[k] > 0.0}


def test_nothing_rendered_reads_zeros(world):
    rec = world.records()
    assert all(v == 0 for v in rec.values()), rec


def test_a_frame_pass_bit_resets_the_seven_pass_records(world):
    gpu, v = world.gpu, world.view()
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    assert frame_passes(world.records()) == set(range(7))
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_DEFERRED)
    assert frame_passes(world.records()) == {GBUFFER, DEFERRED}
    gpu.render_hybrid(v, rr.HYBRID_SKY)
    assert frame_passes(world.records()) == {SKY}
    v.raytracing_supported = 0  # the ray-traced passes are gated, and report 0
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    assert frame_passes(world.records()) == {GBUFFER, SSAO, DEFERRED, SKY, PRESENT}
    v.raytracing_supported, v.ssao_enabled = 1, 0
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    assert frame_passes(world.records()) == set(range(7)) - {SSAO}


def test_a_shadow_map_only_call_keeps_the_pass_records(world):
    gpu, v = world.gpu, world.view()
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_DEFERRED)
    before = world.records()
    assert (before["maps"], before["maps_renders"]) == (0.0, 0)
    gpu.render_hybrid(world.view(shadows_enabled=1), MAPS)
    after = world.records()
    assert after["maps"] > 0.0 and after["maps_renders"] == 1
    assert {k: after[k] for k in after if not k.startswith("maps")} == {k: before[k] for k in before if not k.startswith("maps")}
    assert frame_passes(after) == {GBUFFER, DEFERRED}


def test_an_environment_only_call_resets_the_seven_and_the_environment_records_persist(world):
    gpu, v = world.gpu, world.view()
    gpu.render_hybrid(v, rr.HYBRID_FRAME | ENV)
    rec = world.records()
    assert frame_passes(rec) == set(range(7)) and env_passes(rec) == set(range(4)) and rec["env_builds"] == 1
    gpu.render_hybrid(v, ENV)
    rec = world.records()
    assert frame_passes(rec) == set() and env_passes(rec) == set(range(4)) and rec["env_builds"] == 2
    # later calls without the bit: the last build's records, bit for bit
    for mask in (rr.HYBRID_GBUFFER, rr.HYBRID_FRAME, MAPS):
        gpu.render_hybrid(world.view(shadows_enabled=1 if mask == MAPS else 0), mask)
        after = world.records()
        assert [after[f"env{k}"] for k in range(4)] == [rec[f"env{k}"] for k in range(4)] and after["env_builds"] == 2


def test_the_shadow_maps_bit_without_shadows_reports_zero(world):
    gpu = world.gpu
    gpu.render_hybrid(world.view(shadows_enabled=1), rr.HYBRID_GBUFFER | MAPS)
    rec = world.records()
    assert rec["maps"] > 0.0 and rec["maps_renders"] == 1 and frame_passes(rec) == {GBUFFER}
    gpu.render_hybrid(world.view(shadows_enabled=0), MAPS)  # the mask is the shadow maps' alone: the seven stay
    rec = world.records()
    assert (rec["maps"], rec["maps_renders"]) == (0.0, 1) and frame_passes(rec) == {GBUFFER}
    gpu.render_hybrid(world.view(shadows_enabled=1), MAPS)
    assert world.records()["maps"] > 0.0 and world.records()["maps_renders"] == 2
    gpu.render_hybrid(world.view(shadows_enabled=0), rr.HYBRID_SKY | MAPS)
    rec = world.records()
    assert (rec["maps"], rec["maps_renders"]) == (0.0, 2) and frame_passes(rec) == {SKY}
    gpu.render_hybrid(world.view(shadows_enabled=1), MAPS)
    kept = world.records()["maps"]
    gpu.render_hybrid(world.view(shadows_enabled=1), rr.HYBRID_SKY)  # without the bit the record stays
    assert kept > 0.0 and world.records()["maps"] == kept


def test_the_marching_cubes_bit_with_the_checkbox_off_zeroes_its_record(world):
    gpu = world.gpu
    gpu.render_hybrid(world.view(marching_cubes_enabled=1), rr.HYBRID_GBUFFER | MC)
    rec = world.records()
    assert rec["mc"] > 0.0 and rec["mc_renders"] == 1 and frame_passes(rec) == {GBUFFER}
    gpu.render_hybrid(world.view(marching_cubes_enabled=1), rr.HYBRID_SKY)  # without the bit the record stays
    assert world.records()["mc"] == rec["mc"]
    gpu.render_hybrid(world.view(marching_cubes_enabled=0), rr.HYBRID_SKY)
    assert world.records()["mc"] == rec["mc"]
    gpu.render_hybrid(world.view(marching_cubes_enabled=0), rr.HYBRID_SKY | MC)
    after = world.records()
    assert (after["mc"], after["mc_renders"]) == (0.0, 1) and frame_passes(after) == {SKY}


def test_reservoir_lights_and_rtao_keep_their_reading_without_their_bit(world):
    gpu, v = world.gpu, world.view()
    gpu.render_hybrid(v, rr.HYBRID_FRAME | RESTIR | RTAO)
    rec = world.records()
    assert rec["restir"] > 0.0 and rec["rtao_trace"] > 0.0 and rec["rtao_filter"] > 0.0
    assert frame_passes(rec) == set(range(7)) - {SSAO}, "the rtao pass takes the SSAO slot"
    mine = ("restir", "rtao_trace", "rtao_filter")
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    after = world.records()
    assert [after[k] for k in mine] == [rec[k] for k in mine] and frame_passes(after) == set(range(7))
    gpu.render_hybrid(world.view(ssao_enabled=0), rr.HYBRID_FRAME | RTAO)  # no rtao pass without ssao_enabled: nothing of it is reset
    after = world.records()
    assert [after[k] for k in mine] == [rec[k] for k in mine] and frame_passes(after) == set(range(7)) - {SSAO}
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | RTAO)
    after = world.records()
    assert after["restir"] == rec["restir"] and after["rtao_trace"] > 0.0 and after["rtao_filter"] > 0.0 and frame_passes(after) == {GBUFFER}


def test_motion_and_the_rasterised_g_buffer(world):
    gpu, v = world.gpu, world.view()
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | MOTION)
    rec = world.records()
    assert rec["motion"] > 0.0 and rec["snapshot"] > 0.0 and (rec["raster"], rec["raster_renders"]) == (0.0, 0)
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER | MOTION)
    rec = world.records()
    assert rec["motion"] > 0.0 and rec["raster"] > 0.0 and rec["raster_renders"] == 1  # (no mesh changed: the snapshot stage is empty)
    assert rec["raster"] == rec["frame1"], "the rasterised pass's record is the G-buffer stage's"
    gpu.render_hybrid(v, rr.HYBRID_SKY | MOTION)  # the modifier without the G-buffer pass: ignored
    after = world.records()
    assert (after["motion"], after["snapshot"]) == (rec["motion"], rec["snapshot"]) and after["raster"] == 0.0 and after["raster_renders"] == 1
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    after = world.records()
    assert (after["motion"], after["snapshot"]) == (rec["motion"], rec["snapshot"]) and after["raster"] == 0.0, "a cast G-buffer: no rasterised time"


def test_forward_shadow_maps_move_both_records_together(world):
    gpu = world.gpu
    on, off = world.view(shadows_enabled=1), world.view(shadows_enabled=0)
    gpu.render_forward(on, rr.FORWARD_GRAPH)
    rec = world.records()
    assert rec["maps"] > 0.0 and rec["maps_renders"] == 1 and all(rec[f"forward{k}"] > 0.0 for k in range(3)) and rec["forward_renders"] == 1
    gpu.render_forward(on, rr.FORWARD_PASS | rr.FORWARD_PRESENT)  # the maps of the call before: their record stays, the forward graph's is 0
    after = world.records()
    assert (after["maps"], after["maps_renders"]) == (rec["maps"], 1) and after["forward0"] == 0.0
    assert after["forward1"] > 0.0 and after["forward2"] > 0.0 and after["forward_renders"] == 2
    gpu.render_forward(off, rr.FORWARD_GRAPH)  # the bit without shadows: no render
    after = world.records()
    assert (after["maps"], after["maps_renders"]) == (rec["maps"], 1) and after["forward0"] == 0.0 and after["forward_renders"] == 3
    gpu.render_forward(on, rr.FORWARD_SHADOW_MAPS)
    after = world.records()
    assert after["maps"] > 0.0 and after["forward0"] > 0.0 and after["maps_renders"] == 2
    assert (after["forward1"], after["forward2"], after["forward_renders"]) == (0.0, 0.0, 3)
    assert frame_passes(after) == set(), "the forward graph leaves the hybrid passes' records alone"


def test_a_refused_marching_cubes_pass_changes_no_record(world):
    gpu = world.gpu
    gpu.render_hybrid(world.view(), rr.HYBRID_FRAME)
    before = world.records()
    with pytest.raises(UtopianError, match="the marching-cubes pass: view.num_lights exceeds"):
        gpu.render_hybrid(world.view(marching_cubes_enabled=1, num_lights=3), rr.HYBRID_GBUFFER | rr.HYBRID_SKY | MC)
    assert world.records() == before and (before["mc"], before["mc_renders"]) == (0.0, 0)
    gpu.render_hybrid(world.view(marching_cubes_enabled=1), rr.HYBRID_GBUFFER | rr.HYBRID_SKY | MC)
    rec = world.records()
    assert rec["mc"] > 0.0 and rec["mc_renders"] == 1 and frame_passes(rec) == {GBUFFER, SKY}
    with pytest.raises(UtopianError, match="the marching-cubes pass: view.num_lights exceeds"):
        gpu.render_hybrid(world.view(marching_cubes_enabled=1, num_lights=3), rr.HYBRID_GBUFFER | rr.HYBRID_SKY | MC)
    assert world.records() == rec, "refused before any launch: not even the call's resets"


def test_the_denoiser_s_records_are_its_own(world):
    gpu, v = world.gpu, world.view()
    v.samples_per_frame = v.total_samples = 1
    gpu.render_frame(v, rr.PASS_REFERENCE_PT)
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.denoise(v)
    rec = world.records()
    assert all(rec[f"denoise{k}"] > 0.0 for k in range(4)) and frame_passes(rec) == {GBUFFER}
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    gpu.render_forward(v, rr.FORWARD_PASS)
    after = world.records()
    assert [after[f"denoise{k}"] for k in range(4)] == [rec[f"denoise{k}"] for k in range(4)]
    gpu.denoise(v)
    after2 = world.records()
    assert all(after2[f"denoise{k}"] > 0.0 for k in range(4))
    assert {k: after2[k] for k in after2 if not k.startswith("denoise")} == {k: after[k] for k in after if not k.startswith("denoise")}

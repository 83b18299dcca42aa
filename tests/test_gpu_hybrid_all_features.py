"""GPU: one uh_render_hybrid call with every feature bit against the same passes one call at a time. Two contexts get the same uploads
and the same three frames - between frames the camera shifts and takes the TAA jitter, one instance moves (rebuild_tlas) and view.time
advances. Context A renders each frame as one call with FRAME | SHADOW_MAPS | ENVIRONMENT | GBUFFER_RASTER | MOTION | RESTIR_LIGHTS |
RTAO | MARCHING_CUBES | TAA; context B renders it as separate calls in the pass order of hybrid_passes (csrc/hybrid_graph.hip), and
every pass is held to its own restatement on what B read back before it. After every frame every readable image and every counter of
A equals B's, so a wrong pointer, a stale image or a mis-selected template in the pass table shows in one place or the other.

What hybrid_plan couples within a call, and B therefore keeps together:
  * the deferred pass reads the light-visibility image only with RESTIR_LIGHTS in its own call (plan.restir selects kRestir);
  * the sky pass skips the marching-cubes pixels only with that pass in its own call (plan.mc hands it the visibility);
  * present reads taa_output only with TAA in its own call;
  * MOTION is a modifier of the G-buffer pass and is ignored without it.
The rtao pass runs between restir_lights and the deferred pass in a whole call; neither reads what the other writes (the visibility
image and its counters; the AO counts and ssao_output), so B runs it before the RESTIR_LIGHTS | DEFERRED call."""
import numpy as np
import pytest

import forward_reference as fw
import gbuffer_raster_reference as gr
import hybrid_compose_reference as cr
import hybrid_frame_reference as fr
import hybrid_reference as hr
import hybrid_restir_reference as rl
import ibl_reference as ir
import marching_cubes_pass_reference as mr
import motion_reference as mo
import oracle_api as oa
import rtao_reference as ao
import rust_renderer_amd as rr
import shadow_map_reference as sr
import taa_reference as tr
from hybrid_util import CONSUMER_ULP, DEFERRED_ULP, bits, frame_view, gbuf, ulps
from rust_renderer_amd.scenes import box, icosphere
from test_gpu_denoise import projection_view
from test_gpu_marching_cubes_pass import MarchingCubesScene, _extracted
from test_gpu_motion import MOTION_HELD

pytestmark = pytest.mark.gpu

W, H = 97, 61
FRAMES = 3
SIZE = 256
EXTENT = 56.0  # the floor's width: the scene's extent, to which MOTION_HELD is relative
EYE, TARGET, NEAR, FAR = np.array([-30.0, 28.0, -22.0]), np.array([10.0, 15.0, 10.0]), 5.0, 150.0
METAL, MOVED = 6, 7  # the two meshes added to the marching-cubes scene's six
MOVES = [rr.transform3x4((1.0, 1.0, 1.0), (-6.0 + 2.5 * k, 2.0 + 0.5 * k, 22.0 - 1.5 * k)) for k in range(FRAMES)]
EVERYTHING = (rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS | rr.HYBRID_ENVIRONMENT | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MOTION | rr.HYBRID_RESTIR_LIGHTS |
              rr.HYBRID_RTAO | rr.HYBRID_MARCHING_CUBES | rr.HYBRID_TAA)
IMAGES = range(18)


class EverythingScene(MarchingCubesScene):
    """the marching-cubes scene (the synthetic scene with its metal floor and sphere, a floor under the domain, a quad before it), a large
    metal sphere on the floor and a box that moves from frame to frame"""

    def upload(self, renderer):
        r = super().upload(renderer)
        white = renderer.default_diffuse_map()
        sv, si = icosphere(2)
        assert renderer.add_mesh(sv, si, rr.make_material(rr.METAL, 0.0, (0.9, 0.9, 0.9, 1.0), diffuse_map=white), rr.transform3x4((4.0, 4.0, 4.0), (-14.0, 3.5, 6.0))) == METAL
        bv, bi = box((0.0, 0.0, 0.0), (2.0, 2.5, 2.0))
        assert renderer.add_mesh(bv, bi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.4, 0.3, 1.0), diffuse_map=white), MOVES[0]) == MOVED
        renderer.initialize_raytracing()
        return r


def lights():
    """8 point and spot lights a little above the floor around the box, the metal sphere and the quad, which hide part of the floor from
    each of them"""
    out = []
    for k in range(8):
        a = 2.0 * np.pi * k / 8.0
        l = rr.make_light((-8.0 + 13.0 * np.cos(a), 3.0 + 0.5 * (k % 3), 12.0 + 11.0 * np.sin(a)),
                          color=(2.0 + 6.0 * ((k * 5) % 7) / 6.0, 7.0 - 5.0 * ((k * 3) % 5) / 4.0, 3.0 + 4.0 * (k % 3) / 2.0))
        l.light_type = float(1 + k % 2)
        l.direction[:] = (-np.cos(a), -0.3, -np.sin(a))  # the spot lights look at the middle
        l.spot = 1.0 + (k % 2)
        out.append(l)
    return out


def camera(k):
    """frame k's camera: it moves sideways and down and turns a little toward the floor, so that a strip of each frame was outside the one before"""
    return rr.camera.Camera(tuple(EYE + k * np.array([3.0, -1.0, -2.0])), tuple(TARGET + k * np.array([3.0, -4.0, -2.0])), 60.0, W / H, NEAR, FAR)


def scene_at(k):
    return EverythingScene("everything", [], [], camera(k), dict(sky_enabled=1))


def frame_views(ibl=1):
    """the three views: every flag on, the TAA jitter of the frame's index, the previous frame's un-jittered projection * view; ibl = 0:
    without the IBL maps (ibl_enabled = cubemap_enabled = 0: test_gpu_rtgi_everything.py, whose rtgi pass refuses them)"""
    views, prev = [], None
    for k in range(FRAMES):
        v = frame_view(scene_at(k), W, H, ssao_enabled=1, raytracing_supported=1, fxaa_enabled=1, marching_cubes_enabled=1)
        v.shadows_enabled = 1
        v.ibl_enabled = v.cubemap_enabled = ibl
        v.num_lights, v.time, v.rebuild_tlas = 8, 5.0 + 0.75 * k, 1
        v.samples_per_frame, v.total_samples = 1, k + 1
        pv = projection_view(v)
        v.prev_frame_projection_view[:] = pv if prev is None else prev
        views.append(rr.Renderer.jitter_view(v, k, W, H))
        prev = pv
    return views


class Context:
    """the scene, the lights and three reservoir frames on one renderer; rtao and taa params as the issue sets them"""

    def __init__(self):
        scene = scene_at(0)
        self.gpu = rr.Renderer(W, H)
        self.meshes, self.textures = fw.upload_recorded(scene, self.gpu, defaults=False)
        self.lights = lights()
        for l in self.lights:
            self.gpu.add_gpu_light(l)
        self.gpu.initialize_raytracing()
        loop = rr.FrameLoop(self.gpu, scene.make_view(W, H))
        for _ in range(3):
            loop.frame(rr.PASS_RESTIR)
        self.gpu.set_option("shadow_map_size", SIZE)
        self.rtao = ao.default_params(samples=3)
        self.gpu.set_rtao_params(**self.rtao)
        self.taa = self.gpu.set_taa_params(flags=rr.TAA_CLAMP | rr.TAA_MOTION)

    def begin(self, k, view):
        """what changes between frames, before the frame's first call"""
        if k:
            self.gpu.set_instance_transform(MOVED, MOVES[k])
            self.meshes[MOVED]["world"] = np.ascontiguousarray(MOVES[k], np.float32).reshape(12).copy()
        self.gpu.set_shadowmap_params(rr.shadow_cascades(camera(k), view.sun_dir[:]))

    def images(self):
        g = self.gpu
        out = {i: g.read_hybrid(i) for i in IMAGES}
        out.update({f"shadow map {c}": g.read_shadow_map(c) for c in range(4)})
        maps = ir.read_maps(g)
        out.update({f"env {m}": a for m, a in enumerate(maps["env"])})
        out.update({f"spec {m}": a for m, a in enumerate(maps["spec"])})
        out.update(irr=maps["irr"], lut=maps["lut"])
        return out


def _affine4(m3x4):
    return np.concatenate([np.asarray(m3x4, np.float64).reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]]])


def counters(gpu, *which):
    """the counters of the stats structs (no times), by group"""
    get = dict(
        shadow_maps=lambda: (lambda s: (s.renders, s.size, tuple(s.triangles), bytes(s.params)))(gpu.shadow_map_stats()),
        shadows=lambda: (gpu.hybrid_stats().rays[1],),
        gbuffer=lambda: (gpu.hybrid_stats().rays[0],) + (lambda s: (s.renders, s.pieces, s.covered_pixels))(gpu.gbuffer_raster_stats()),
        motion=lambda: (lambda s: (s.pixels_with, s.pixels_without, s.meshes_static, s.meshes_rigid, s.meshes_deformed, s.meshes_none))(gpu.motion_stats()),
        env=lambda: (lambda s: (s.builds, tuple(s.sun_dir), tuple(s.eye)))(gpu.environment_stats()),
        reflections=lambda: (gpu.hybrid_stats().rays[2], gpu.hybrid_stats().reflection_pixels),
        restir=lambda: (lambda s: (s.rays, s.occluded))(gpu.hybrid_restir_stats()),
        rtao=lambda: (lambda s: (s.pixels, s.rays, s.occluded))(gpu.rtao_stats()),
        deferred=lambda: (gpu.hybrid_frame_stats().lights,),
        mc=lambda: (lambda s: (s.renders, s.triangles, s.pieces, s.covered_pixels, s.lights, s.time))(gpu.marching_cubes_stats()),
        sky=lambda: (gpu.hybrid_frame_stats().sky_pixels,),
        taa=lambda: (lambda s: (s.history_pixels, s.reset_pixels))(gpu.taa_stats()))
    return {k: get[k]() for k in (which or get)}


@pytest.fixture(scope="module")
def world():
    a, b = Context(), Context()
    assert np.array_equal(a.gpu.read_reservoirs(2).view(np.uint8), b.gpu.read_reservoirs(2).view(np.uint8)), "the same reservoir frames"
    cpu = oa.OracleRenderer(W, H)
    hr.upload_recorded(scene_at(0), cpu, False)
    for l in a.lights:
        cpu.add_gpu_light(l)
    cpu.initialize_raytracing()
    return a, b, cpu


def separate_calls(b, cpu, k, v, taa_ref):
    """frame k on context B, one call per pass (or per coupled group), each pass held to its restatement on B's own read-backs.
    Returns the counters collected after the calls that produce them and what frame three's coverage conditions need"""
    gpu, meshes, textures, lights_ = b.gpu, b.meshes, b.textures, b.lights
    read = gpu.read_hybrid
    count, seen = {}, {}
    # -- setup_shadow_pass: bit for bit
    gpu.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    count.update(counters(gpu, "shadow_maps"))
    params = gpu.shadow_map_stats().params
    smaps = np.stack([gpu.read_shadow_map(c) for c in range(4)])
    want = sr.shadow_maps(meshes, params, SIZE)
    assert np.array_equal(bits(smaps), bits(want)), f"frame {k}: shadow maps"
    shadow = (params, smaps)
    # -- rt_shadows on the previous frame's G-buffer (compared with A's below)
    gpu.render_hybrid(v, rr.HYBRID_RT_SHADOWS)
    count.update(counters(gpu, "shadows"))
    # -- the rasterised G-buffer with the motion pass
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_GBUFFER_RASTER | rr.HYBRID_MOTION)
    count.update(counters(gpu, "gbuffer", "motion"))
    g = gbuf(gpu)
    ref = gr.gbuffer_raster(meshes, textures, v, W, H)
    gdepth, gvis = read(rr.HYBRID_GBUFFER_DEPTH), read(rr.HYBRID_GBUFFER_VISIBILITY)
    assert np.array_equal(gvis, ref["visibility"]) and np.array_equal(bits(gdepth), bits(ref["depth"])), f"frame {k}: raster depth / visibility"
    for key in ("position", "normal", "pbr"):
        assert np.array_equal(bits(g[key]), bits(ref[key])), f"frame {k}: {key}"
    assert np.array_equal(g["albedo"], ref["albedo"]), f"frame {k}: albedo"
    pos, geo = g["position"], g["position"][..., 3] != 0
    mesh = np.where(geo, g["pbr"][..., 3], -1.0)
    motion = read(rr.HYBRID_MOTION_IMAGE)
    moved = geo & (mesh == MOVED)
    rigid = moved if k else np.zeros_like(moved)
    still = geo & ~rigid
    assert np.array_equal(bits(motion[..., :3])[still], bits(pos[..., :3])[still]) and (motion[..., 3][geo] == 1).all() and not motion[~geo].any(), f"frame {k}: motion"
    if k:
        prev_to_now = mo.affine((_affine4(MOVES[k - 1]) @ _affine4(mo.inverse3x4(MOVES[k])))[:3], pos[..., :3])  # where the point was a frame ago
        assert moved.sum() >= 20 and float(np.abs(prev_to_now[moved] - pos[..., :3][moved]).max()) > 0.5, "the box is on screen and moved"
        e = float(np.abs(motion[..., :3][moved].astype(np.float64) - prev_to_now[moved]).max()) / EXTENT
        assert e <= MOTION_HELD, f"frame {k}: motion of the moved box {e:.3e}"
    # -- setup_cubemap_pass (compared with A's below), then rt_reflections with IBL
    gpu.render_hybrid(v, rr.HYBRID_ENVIRONMENT)
    count.update(counters(gpu, "env"))
    maps = ir.read_maps(gpu)
    gpu.render_hybrid(v, rr.HYBRID_RT_REFLECTIONS)
    count.update(counters(gpu, "reflections"))
    refl = read(rr.HYBRID_REFLECTIONS)
    want, kind = ir.reflections_ibl(cpu, meshes, g["position"], g["normal"], g["pbr"], v, maps)
    assert np.abs(refl.astype(int) - want.astype(int)).max() <= 1, f"frame {k}: reflections"
    # -- the rtao pass
    gpu.render_hybrid(v, rr.HYBRID_RTAO)
    count.update(counters(gpu, "rtao"))
    ao_count, ss = read(rr.HYBRID_AO_COUNTS), read(rr.HYBRID_SSAO_IMAGE)
    want_count, totals, want_img = ao.image(cpu, g, v, b.rtao)
    assert np.array_equal(ao_count, want_count) and count["rtao"] == totals and np.array_equal(ss, want_img), f"frame {k}: rtao"
    # -- restir_lights and the deferred pass that reads its image
    gpu.render_hybrid(v, rr.HYBRID_RESTIR_LIGHTS | rr.HYBRID_DEFERRED)
    count.update(counters(gpu, "restir", "deferred"))
    res, vis = gpu.read_reservoirs(2), read(rr.HYBRID_LIGHT_VISIBILITY)
    want_vis, rays, occluded = rl.visibility(cpu, g, res, v, lights_)
    assert np.array_equal(vis, want_vis) and count["restir"] == (rays, occluded), f"frame {k}: light visibility"
    deferred = read(rr.HYBRID_DEFERRED_OUTPUT)
    sh = read(rr.HYBRID_SHADOWS)
    want = cr.deferred(g, sh, refl, ss, v, meshes, lights_, maps=maps, shadow=shadow, res=res, vis=vis)
    assert np.isfinite(deferred[geo]).all() and ulps(deferred[geo][:, :3], want[geo][:, :3]).max() <= CONSUMER_ULP, f"frame {k}: deferred"
    # -- the marching-cubes pass over that image, and the sky around it
    gpu.render_hybrid(v, rr.HYBRID_MARCHING_CUBES | rr.HYBRID_SKY)
    count.update(counters(gpu, "mc", "sky"))
    out = read(rr.HYBRID_DEFERRED_OUTPUT)
    mpos, mnrm = _extracted(v.time)
    ref = mr.marching_cubes_pass(mr.pass_mesh(mpos, mnrm, meshes[0]), textures, v, lights_, pos, deferred, shadow, seed=gdepth)
    mvis = read(rr.HYBRID_MARCHING_CUBES_VISIBILITY)
    assert np.array_equal(mvis, ref["visibility"]) and np.array_equal(bits(read(rr.HYBRID_DEPTH)), bits(ref["depth"])), f"frame {k}: marching-cubes depth / visibility"
    covered = mvis != mr.NONE
    assert ulps(out[covered], ref["output"][covered]).max() <= DEFERRED_ULP, f"frame {k}: marching-cubes colour"
    sky = ~geo & ~covered
    assert np.array_equal(bits(out[geo & ~covered]), bits(deferred[geo & ~covered])), f"frame {k}: geometry pixels the pass did not draw stay"
    cube = ir.sky_cube(np.where(sky[..., None], pos, np.float32(1.0)), v, maps["env"])
    assert len(cube) == int(sky.sum()) == count["sky"][0], f"frame {k}: sky pixels"
    ys, xs = np.array(list(cube)).T
    assert np.allclose(out[ys, xs, :3], np.array(list(cube.values()), np.float32), rtol=1e-5, atol=1e-7) and (out[ys, xs, 3] == 1.0).all(), f"frame {k}: sky"
    # -- the taa pass and present on its output
    gpu.render_hybrid(v, rr.HYBRID_TAA | rr.HYBRID_PRESENT)
    count.update(counters(gpu, "taa"))
    taa_out, taa_n = read(rr.HYBRID_TAA_OUTPUT), read(rr.HYBRID_TAA_HISTORY)
    want = taa_ref(out, pos, motion, v, tr.params_of(b.taa), W, H)
    assert np.array_equal(bits(taa_out), bits(want["output"])) and np.array_equal(bits(taa_n), bits(want["history"])), f"frame {k}: taa"
    assert count["taa"] == (want["history_pixels"], want["reset_pixels"])
    assert np.array_equal(read(rr.HYBRID_PRESENT_OUTPUT), fr.present(taa_out, True)), f"frame {k}: present"
    typ = np.array([m["type"] for m in meshes] + [0.0], np.float32)[np.minimum(g["pbr"][..., 3].astype(np.uint32), len(meshes))]
    cast = rl.cast_mask(g, res, v, lights_)
    unseeded = fw.resolve(ref["records"], W, H)[1] != mr.NONE
    seen.update(sky=int(sky.sum()), metal=int((geo & (typ == 1.0)).sum()), lit=int((vis[cast] == 255).sum()), occluded=int((vis[cast] == 0).sum()),
                ao=set(np.unique(ao_count[geo]).tolist()), iso_over_sky=int((covered & ~geo).sum()), iso_hidden=int((unseeded & ~covered & geo).sum()),
                taa=count["taa"], rigid=count["motion"][3])
    return count, seen


def test_one_call_with_everything_equals_the_passes_one_at_a_time(world):
    a, b, cpu = world
    taa_ref = tr.Taa()
    for k, v in enumerate(frame_views()):
        for c in (a, b):
            c.begin(k, v)
        if k:
            cpu.set_instance_transform(MOVED, MOVES[k])
            cpu.initialize_raytracing()
        a.gpu.render_hybrid(v, EVERYTHING)
        want_count, seen = separate_calls(b, cpu, k, v, taa_ref)
        got, want = a.images(), b.images()
        for name in want:
            assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), f"frame {k}: image {name} of the one call differs from the separate calls'"
        got_count = counters(a.gpu)
        assert got_count == want_count, f"frame {k}: {[(n, got_count[n], want_count[n]) for n in want_count if got_count[n] != want_count[n]]}"
    print(f"frame {FRAMES}: {seen}")
    assert seen["sky"] > 0 and seen["metal"] > 0 and seen["lit"] > 0 and seen["occluded"] > 0 and len(seen["ao"]) > 1
    assert seen["iso_over_sky"] > 0 and seen["iso_hidden"] > 0, "the isosurface in front of the sky and hidden behind geometry"
    assert seen["taa"][0] > 0 and seen["taa"][1] > 0 and seen["rigid"] == 1

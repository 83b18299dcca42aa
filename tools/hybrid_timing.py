"""Timing of the hybrid graph (uh_render_hybrid) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's two spheres, one
metal), camera at rest, warm: the hipEvent ms of each pass, median of --iters calls. Prints one JSON line per measurement. --mode picks
what is timed:

  passes  the ray-traced passes (UH_HYBRID_ALL, IBL off): ms, rays per pass and metal pixels
  frame   the whole frame (UH_HYBRID_FRAME: rt_shadows, G-buffer, rt_reflections, SSAO, deferred, sky, present; IBL off) with each light
          count of --lights (1,024: the light count of BASELINE config 2; point and spot lights alternate)
  ibl     the IBL maps (UH_HYBRID_ENVIRONMENT: environment cube, irradiance cube, specular cube, BRDF LUT), median of --builds builds,
          then the whole frame with IBL off and with the reference's flags (ibl_enabled = cubemap_enabled = 1, shadows_enabled = 0)
  shadows the cascaded shadow maps (UH_HYBRID_SHADOW_MAPS at the default 4096^2, uh_shadow_cascades of the scene's camera and sun),
          median of --builds renders, with the triangles per cascade; the whole frame with shadows_enabled = 0 and 1 (maps rendered
          once); the whole frame with the reference's default flags (shadows_enabled = ibl_enabled = cubemap_enabled = 1, the IBL
          and shadow maps built once), and the same frame with the shadow maps re-rendered in every call, as the reference does
  forward the forward graph (uh_render_forward: shadow maps, forward pass, present) with each light count of --lights and
          shadows_enabled = 0, then shadows_enabled = 1 with the maps re-rendered in every call (the reference's key 3), beside the
          hybrid G-buffer cast + deferred pass of the same view
  marching_cubes  the marching-cubes pass (UH_HYBRID_MARCHING_CUBES, marching_cubes_enabled = 1, view.time 5) in the whole frame,
          with shadows_enabled = 0 and 1 (maps rendered once): the pass's ms, its triangles, pieces and covered pixels, and the frame's
          passes beside it; then the same on a scene of one floor with the isosurface in full view
  gbuffer_raster  the G-buffer pass rasterised (UH_HYBRID_GBUFFER | UH_HYBRID_GBUFFER_RASTER) alone, with its pieces and covered
          pixels, beside the cast alone; then the whole frame (UH_HYBRID_FRAME, IBL and shadows off) with the rasterised and with the
          cast G-buffer
  restir_lights  on config 2's scene class (the same scene with 1,024 point lights), for each light count of --lights as view.num_lights:
          the reservoir passes (uh_render_frame with UH_PASS_RESTIR: G-buffer cast, initial RIS, temporal and spatial reuse) as
          UhStats.last_frame_ms; the whole frame with UH_HYBRID_RESTIR_LIGHTS - the restir_lights pass (UhHybridRestirStats, with its rays
          and occluded rays) and the deferred pass that adds one light per pixel - beside the whole frame without the bit, whose deferred
          pass loops over all the lights unshadowed. With UTOPIAN_HIP_LIB naming a library from before the bit existed (the parent
          commit's), the reservoir passes and the plain frame alone

Run it under `rocprofv3 --kernel-trace --stats -- python tools/hybrid_timing.py --mode ...` for the kernel table.

  python tools/hybrid_timing.py [--mode passes|frame|ibl|shadows|forward|marching_cubes|gbuffer_raster|restir_lights --width 1920 --height 1080 --warmup 3 --iters 20 --lights 0,16,1024
                                 --builds 5 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_renderer_amd as rr  # noqa: E402

PASSES = ("rt_shadows", "gbuffer", "rt_reflections", "ssao", "deferred", "sky", "present")
SUBPASSES = ("environment", "irradiance", "specular", "brdf_lut")


def add_lights(r, n, seed=11):
    rng = np.random.default_rng(seed)
    for k in range(n):
        l = rr.make_light(rng.uniform((-12.0, 0.5, -5.0), (12.0, 10.0, 5.0)), color=tuple(rng.uniform(0.2, 1.0, 3)))
        l.light_type = 1.0 if k % 2 == 0 else 2.0
        l.direction[:] = (0.0, -1.0, 0.0)
        l.spot = 8.0
        r.add_gpu_light(l)


def setup(a, lights=0, **flags):
    """the scene on a new renderer with `lights` lights, its view with `flags` set, and the path tracer's camera grid for this camera
    (two frames at rest): the G-buffer cast goes through it, as it does in a frame"""
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    if lights:
        add_lights(r, lights)
        r.initialize_raytracing()
    view = scene.make_view(a.width, a.height)
    for k, v in flags.items():
        setattr(view, k, v)
    for _ in range(2):
        r.render_frame(view, rr.PASS_GBUFFER)
    return scene, r, view


def timed(a, r, view, mask, stats):
    """--warmup calls, then --iters calls each followed by stats(r), which waits (one call at a time on an idle GPU): the median of
    each pass_ms entry and the last call's stats"""
    for _ in range(a.warmup):
        r.render_hybrid(view, mask)
    per = []
    for _ in range(a.iters):
        r.render_hybrid(view, mask)
        per.append(stats(r))
    ms = [list(s.pass_ms) for s in per]
    return [statistics.median(m[k] for m in ms) for k in range(len(ms[0]))], per[-1]


def passes(a):
    scene, r, view = setup(a, ibl_enabled=0)
    med, s = timed(a, r, view, rr.HYBRID_ALL, rr.Renderer.hybrid_stats)
    yield dict(metric="hybrid_frame", config=1, width=a.width, height=a.height, iters=a.iters,
               gbuffer_ms=med[0], rt_shadows_ms=med[1], rt_reflections_ms=med[2], total_ms=sum(med),
               rays=dict(zip(("gbuffer", "shadow", "reflection"), list(s.rays))), metal_pixels=s.reflection_pixels,
               camera_grid=r.get_stats().camera_grid_cells > 0, triangles=scene.num_triangles)


def frame(a):
    for n in (int(x) for x in a.lights.split(",")):
        scene, r, view = setup(a, n, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0, num_lights=n)
        med, s = timed(a, r, view, rr.HYBRID_FRAME, rr.Renderer.hybrid_frame_stats)
        yield dict(metric="hybrid_frame_full", config=1, lights=n, width=a.width, height=a.height, iters=a.iters,
                   **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med), sky_pixels=s.sky_pixels, triangles=scene.num_triangles)


def ibl(a):
    _, r, view = setup(a, shadows_enabled=0, num_lights=0)
    builds = []
    for _ in range(a.builds):
        r.render_hybrid(view, rr.HYBRID_ENVIRONMENT)
        builds.append(list(r.environment_stats().pass_ms))  # waits: one build at a time on an idle GPU
    med = [statistics.median(b[k] for b in builds) for k in range(4)]
    yield dict(metric="ibl_environment_update", builds=a.builds, **{f"{p}_ms": m for p, m in zip(SUBPASSES, med)}, total_ms=sum(med),
               first_build_ms=sum(builds[0]))
    for on in (0, 1):
        view.ibl_enabled = view.cubemap_enabled = on
        med, _ = timed(a, r, view, rr.HYBRID_FRAME, rr.Renderer.hybrid_frame_stats)
        yield dict(metric="hybrid_frame_full", config=1, lights=0, ibl=on, width=a.width, height=a.height, iters=a.iters,
                   **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med))


def shadows(a):
    scene, r, view = setup(a, shadows_enabled=1, ibl_enabled=0, cubemap_enabled=0, num_lights=0)
    r.set_shadowmap_params(rr.shadow_cascades(scene.camera, view.sun_dir[:]))
    renders = []
    for _ in range(a.builds):
        r.render_hybrid(view, rr.HYBRID_SHADOW_MAPS)
        renders.append(r.shadow_map_stats())  # waits: one render at a time on an idle GPU
    s = renders[-1]
    yield dict(metric="shadow_maps", config=1, size=s.size, renders=a.builds, pass_ms=statistics.median(x.pass_ms for x in renders),
               first_render_ms=renders[0].pass_ms, triangles_per_cascade=list(s.triangles), triangles=scene.num_triangles)
    for on in (0, 1):
        view.shadows_enabled = on
        med, _ = timed(a, r, view, rr.HYBRID_FRAME, rr.Renderer.hybrid_frame_stats)
        yield dict(metric="hybrid_frame_full", config=1, lights=0, shadows=on, width=a.width, height=a.height, iters=a.iters,
                   **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med))
    view.shadows_enabled = view.ibl_enabled = view.cubemap_enabled = 1
    r.render_hybrid(view, rr.HYBRID_ENVIRONMENT)
    med, _ = timed(a, r, view, rr.HYBRID_FRAME, rr.Renderer.hybrid_frame_stats)
    yield dict(metric="hybrid_frame_full", config=1, lights=0, reference_defaults=True, width=a.width, height=a.height, iters=a.iters,
               **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med))

    class Both:  # the seven passes and the shadow-map pass of one call
        def __init__(self, r):
            self.pass_ms = list(r.hybrid_frame_stats().pass_ms) + [r.shadow_map_stats().pass_ms]

    # the reference re-renders the cascades every frame (setup_shadow_pass runs in every graph build): the per-frame cost
    med, _ = timed(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS, Both)
    yield dict(metric="hybrid_frame_full", config=1, lights=0, reference_defaults=True, shadow_maps_every_frame=True, width=a.width,
               height=a.height, iters=a.iters, **{f"{p}_ms": m for p, m in zip(PASSES + ("shadow_maps",), med)}, total_ms=sum(med))


def forward(a):
    for n in (int(x) for x in a.lights.split(",")):
        scene, r, view = setup(a, n, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0, num_lights=n)
        for shadows in (0, 1):
            view.shadows_enabled = shadows
            if shadows:
                r.set_shadowmap_params(rr.shadow_cascades(scene.camera, view.sun_dir[:]))
            for _ in range(a.warmup):
                r.render_forward(view)
            per = []
            for _ in range(a.iters):
                r.render_forward(view)
                per.append(r.forward_stats())  # waits: one call at a time on an idle GPU
            med = [statistics.median(s.pass_ms[k] for s in per) for k in range(3)]
            s = per[-1]
            yield dict(metric="forward_graph", config=1, lights=n, shadows=shadows, width=a.width, height=a.height, iters=a.iters,
                       shadow_maps_ms=med[0], forward_ms=med[1], present_ms=med[2], total_ms=sum(med), pieces=s.pieces,
                       covered_pixels=s.covered_pixels, triangles=scene.num_triangles)
        view.shadows_enabled = 0
        med, _ = timed(a, r, view, rr.HYBRID_GBUFFER | rr.HYBRID_DEFERRED, rr.Renderer.hybrid_frame_stats)
        yield dict(metric="hybrid_gbuffer_deferred", config=1, lights=n, width=a.width, height=a.height, iters=a.iters,
                   gbuffer_ms=med[1], deferred_ms=med[4], total_ms=med[1] + med[4])


def _mc_timed(a, r, view, scene_name):
    for _ in range(a.warmup):
        r.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_MARCHING_CUBES)
    per, frames = [], []
    for _ in range(a.iters):
        r.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_MARCHING_CUBES)
        per.append(r.marching_cubes_stats())  # waits: one call at a time on an idle GPU
        frames.append(r.hybrid_frame_stats())
    med = [statistics.median(f.pass_ms[k] for f in frames) for k in range(len(PASSES))]
    s = per[-1]
    mc = statistics.median(p.pass_ms for p in per)
    return dict(metric="hybrid_marching_cubes", scene=scene_name, lights=0, shadows=view.shadows_enabled, width=a.width, height=a.height,
                iters=a.iters, marching_cubes_ms=mc, triangles=s.triangles, pieces=s.pieces, covered_pixels=s.covered_pixels,
                **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med) + mc)


def marching_cubes(a):
    scene, r, view = setup(a, 0, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0, num_lights=0)
    view.marching_cubes_enabled, view.time = 1, 5.0
    for shadows in (0, 1):
        view.shadows_enabled = shadows
        if shadows:
            r.set_shadowmap_params(rr.shadow_cascades(scene.camera, view.sun_dir[:]))
            r.render_hybrid(view, rr.HYBRID_SHADOW_MAPS)
        yield _mc_timed(a, r, view, "config 1")
    # the isosurface in full view: one floor under the domain [0, 32]^3, the camera aimed at (10, 15, 10)
    r = rr.Renderer(a.width, a.height)
    m = rr.make_material(rr.LAMBERTIAN, 0.0, (0.7, 0.7, 0.7, 1.0), diffuse_map=r.default_diffuse_map())
    fv, fi = rr.scenes.quad((-12.0, -0.5, 44.0), (56.0, 0.0, 0.0), (0.0, 0.0, -56.0), nu=4, nv=4)
    r.add_mesh(fv, fi, m)
    r.initialize_raytracing()
    cam = rr.camera.Camera((-30.0, 28.0, -22.0), (10.0, 15.0, 10.0), 60.0, a.width / a.height, 0.1, 1000.0)
    view = rr.default_view(cam, a.width, a.height)
    view.shadows_enabled = view.ibl_enabled = view.cubemap_enabled = 0
    view.marching_cubes_enabled, view.time = 1, 5.0
    yield _mc_timed(a, r, view, "floor and isosurface")


def gbuffer_raster(a):
    scene, r, view = setup(a, 0, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0, num_lights=0)
    for raster in (1, 0):
        mask = rr.HYBRID_GBUFFER | (rr.HYBRID_GBUFFER_RASTER if raster else 0)
        med, _ = timed(a, r, view, mask, rr.Renderer.hybrid_frame_stats)
        line = dict(metric="hybrid_gbuffer", config=1, rasterised=bool(raster), width=a.width, height=a.height, iters=a.iters, gbuffer_ms=med[1],
                    triangles=scene.num_triangles)
        if raster:
            s = r.gbuffer_raster_stats()
            line.update(pieces=s.pieces, covered_pixels=s.covered_pixels)
        yield line
    for raster in (1, 0):
        mask = rr.HYBRID_FRAME | (rr.HYBRID_GBUFFER_RASTER if raster else 0)
        med, _ = timed(a, r, view, mask, rr.Renderer.hybrid_frame_stats)
        yield dict(metric="hybrid_frame_full", config=1, lights=0, gbuffer_rasterised=bool(raster), width=a.width, height=a.height, iters=a.iters,
                   **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med))


def restir_lights(a):
    scene = rr.scenes.scene_for_config(2, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    for n in (int(x) for x in a.lights.split(",")):
        if not 0 < n <= r.get_num_lights():
            continue
        view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
        view.num_lights = n
        frame_ms = []
        for k in range(a.warmup + a.iters):  # a camera at rest: the temporal pass reprojects onto the same pixel
            view.total_samples += 1
            r.render_frame(view, rr.PASS_RESTIR)
            frame_ms.append(r.get_stats().last_frame_ms)  # waits
        line = dict(metric="hybrid_restir_lights", config=2, lights=n, width=a.width, height=a.height, iters=a.iters, triangles=scene.num_triangles,
                    reservoir_passes_ms=statistics.median(frame_ms[a.warmup:]))

        class Both:  # the seven passes and the restir_lights pass of one call
            def __init__(self, r):
                self.restir = r.hybrid_restir_stats()
                self.pass_ms = list(r.hybrid_frame_stats().pass_ms) + [self.restir.pass_ms]

        med, _ = timed(a, r, view, rr.HYBRID_FRAME, rr.Renderer.hybrid_frame_stats)
        line.update(deferred_all_lights_ms=med[4], frame_all_lights_ms=sum(med))
        if not hasattr(r._lib, "uh_get_hybrid_restir_stats"):  # UTOPIAN_HIP_LIB names a library from before the bit: the plain frame alone
            yield line
            continue
        med, s = timed(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_RESTIR_LIGHTS, Both)
        line.update(restir_lights_ms=med[7], deferred_with_bit_ms=med[4], frame_with_bit_ms=sum(med), rays=s.restir.rays, occluded=s.restir.occluded)
        line["reservoir_path_ms"] = line["reservoir_passes_ms"] + line["restir_lights_ms"] + line["deferred_with_bit_ms"]
        line["reservoir_path_faster"] = line["reservoir_path_ms"] < line["deferred_all_lights_ms"]
        yield line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("passes", "frame", "ibl", "shadows", "forward", "marching_cubes", "gbuffer_raster", "restir_lights"),
                    default="passes")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lights", default="0,16,1024", help="frame, forward, restir_lights: the light counts")
    ap.add_argument("--builds", type=int, default=5, help="ibl: the map builds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for out in {"passes": passes, "frame": frame, "ibl": ibl, "shadows": shadows, "forward": forward, "marching_cubes": marching_cubes,
                "gbuffer_raster": gbuffer_raster, "restir_lights": restir_lights}[a.mode](a):
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

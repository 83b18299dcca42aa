"""Timing of the hybrid graph's whole frame (uh_render_hybrid with UH_HYBRID_FRAME: rt_shadows, G-buffer, rt_reflections, SSAO, deferred,
sky, present) at 1920 x 1080, camera at rest, warm: the hipEvent ms of each pass, median of --iters calls, for the config-1 scene
(Sponza-class with the reference's two spheres) with 0, 16 and 1,024 lights (the light count of BASELINE config 2; point and spot
lights alternate). Prints one JSON line per light count. Run it under `rocprofv3 --kernel-trace --stats -- python
tools/hybrid_frame_timing.py` for the kernel table.

  python tools/hybrid_frame_timing.py [--lights 0,16,1024 --warmup 3 --iters 20 --out FILE]"""
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


def add_lights(r, n, seed=11):
    rng = np.random.default_rng(seed)
    for k in range(n):
        l = rr.make_light(rng.uniform((-12.0, 0.5, -5.0), (12.0, 10.0, 5.0)), color=tuple(rng.uniform(0.2, 1.0, 3)))
        l.light_type = 1.0 if k % 2 == 0 else 2.0
        l.direction[:] = (0.0, -1.0, 0.0)
        l.spot = 8.0
        r.add_gpu_light(l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lights", default="0,16,1024")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in (int(x) for x in a.lights.split(",")):
        scene = rr.scenes.scene_for_config(1, with_spheres=True)
        r = scene.upload(rr.Renderer(a.width, a.height))
        if n:
            add_lights(r, n)
            r.initialize_raytracing()
        view = scene.make_view(a.width, a.height)
        view.shadows_enabled = view.ibl_enabled = view.cubemap_enabled = 0
        view.num_lights = n
        for _ in range(2):  # the path tracer's camera grid for this camera: the G-buffer cast goes through it
            r.render_frame(view, rr.PASS_GBUFFER)
        for _ in range(a.warmup):
            r.render_hybrid(view, rr.HYBRID_FRAME)
        per = []
        for _ in range(a.iters):
            r.render_hybrid(view, rr.HYBRID_FRAME)
            per.append(list(r.hybrid_frame_stats().pass_ms))  # waits: one call at a time on an idle GPU
        med = [statistics.median(p[k] for p in per) for k in range(7)]
        s = r.hybrid_frame_stats()
        out = dict(metric="hybrid_frame_full", config=1, lights=n, width=a.width, height=a.height, iters=a.iters,
                   **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med), sky_pixels=s.sky_pixels, triangles=scene.num_triangles)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

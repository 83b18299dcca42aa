"""Timing of the hybrid graph's ray-traced passes (uh_render_hybrid) on the config-1 scene (Sponza-class with the reference's two
spheres, one metal) at 1920 x 1080, camera at rest, UH_HYBRID_ALL, warm: hipEvent ms of each pass, rays per pass and metal pixels.
Prints one JSON line. Run it under `rocprofv3 --kernel-trace --stats -- python tools/hybrid_timing.py` for the kernel table.

  python tools/hybrid_timing.py [--width 1920 --height 1080 --warmup 3 --iters 20 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_renderer_amd as rr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height)
    view.ibl_enabled = 0
    # the path tracer's camera grid for this camera (two frames at rest): the G-buffer cast goes through it, as it does in a frame
    for _ in range(2):
        r.render_frame(view, rr.PASS_GBUFFER)
    for _ in range(a.warmup):
        r.render_hybrid(view, rr.HYBRID_ALL)
    per = []
    for _ in range(a.iters):
        r.render_hybrid(view, rr.HYBRID_ALL)
        s = r.hybrid_stats()  # waits: one call at a time on an idle GPU
        per.append((list(s.pass_ms), list(s.rays), s.reflection_pixels))
    med = [statistics.median(p[0][k] for p in per) for k in range(3)]
    out = dict(metric="hybrid_frame", config=1, width=a.width, height=a.height, iters=a.iters,
               gbuffer_ms=med[0], rt_shadows_ms=med[1], rt_reflections_ms=med[2], total_ms=sum(med),
               rays=dict(zip(("gbuffer", "shadow", "reflection"), per[-1][1])), metal_pixels=per[-1][2],
               camera_grid=r.get_stats().camera_grid_cells > 0, triangles=scene.num_triangles)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

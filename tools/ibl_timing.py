"""Timing of the IBL maps (uh_render_hybrid with UH_HYBRID_ENVIRONMENT: environment cube, irradiance cube, specular cube, BRDF LUT) and
of the hybrid graph's whole frame with them at 1920 x 1080, camera at rest, warm, for the config-1 scene (Sponza-class with the
reference's two spheres): the hipEvent ms of each build sub-pass, median of --builds builds, then the frame's passes with the reference's
flags (ibl_enabled = cubemap_enabled = 1, shadows_enabled = 0) next to the same frame with IBL off, median of --iters calls. Prints one
JSON line per measurement. Run it under `rocprofv3 --kernel-trace --stats -- python tools/ibl_timing.py` for the kernel table.

  python tools/ibl_timing.py [--builds 5 --warmup 3 --iters 20 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_renderer_amd as rr  # noqa: E402

SUBPASSES = ("environment", "irradiance", "specular", "brdf_lut")
PASSES = ("rt_shadows", "gbuffer", "rt_reflections", "ssao", "deferred", "sky", "present")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height)
    view.shadows_enabled = 0
    view.num_lights = 0
    for _ in range(2):  # the path tracer's camera grid for this camera: the G-buffer cast goes through it
        r.render_frame(view, rr.PASS_GBUFFER)
    builds = []
    for _ in range(a.builds):
        r.render_hybrid(view, rr.HYBRID_ENVIRONMENT)
        builds.append(list(r.environment_stats().pass_ms))  # waits: one build at a time on an idle GPU
    med = [statistics.median(b[k] for b in builds) for k in range(4)]
    lines.append(json.dumps(dict(metric="ibl_environment_update", builds=a.builds, **{f"{p}_ms": m for p, m in zip(SUBPASSES, med)}, total_ms=sum(med),
                                 first_build_ms=sum(builds[0]))))
    print(lines[-1], flush=True)
    for ibl in (0, 1):
        view.ibl_enabled = view.cubemap_enabled = ibl
        for _ in range(a.warmup):
            r.render_hybrid(view, rr.HYBRID_FRAME)
        per = []
        for _ in range(a.iters):
            r.render_hybrid(view, rr.HYBRID_FRAME)
            per.append(list(r.hybrid_frame_stats().pass_ms))
        med = [statistics.median(p[k] for p in per) for k in range(7)]
        lines.append(json.dumps(dict(metric="hybrid_frame_full", config=1, lights=0, ibl=ibl, width=a.width, height=a.height, iters=a.iters,
                                     **{f"{p}_ms": m for p, m in zip(PASSES, med)}, total_ms=sum(med))))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

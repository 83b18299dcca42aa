"""Timing of the hybrid frame's area lights (UH_HYBRID_AREA_LIGHTS) at 1920 x 1080 on the Cornell scene (its ceiling lamp is a box of
material type 3: twelve emitter triangles), warm, through the Python layer: the stage times of UhAreaLightStats (the table build, classify
+ sampling, the shadow rays' any-hit walk, means + filter, composite) with the pass's totals at 1, 2 and 16 samples for both item orders of
the sample kernel ("area_light_order" 0, 1: area_lights.hip), next to the whole uh_render_hybrid(HYBRID_FRAME [| HYBRID_AREA_LIGHTS]) call
from its start to the end of a wait behind it. Each figure is the median of --iters calls with a wait after each; the spread (max - min)
is recorded next to it.

  python tools/area_light_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDERS = {0: "a_pixels_samples_together", 1: "one_sample_of_consecutive_pixels"}
STAGES = ("sample_ms", "shadow_ms", "filter_ms", "composite_ms")


def timed_calls(a, rr, r, view, mask):
    rows = dict(call_ms=[], **{k: [] for k in STAGES})
    on = mask & rr.HYBRID_AREA_LIGHTS
    for _ in range(a.warmup + a.iters):
        r.synchronize()
        t0 = time.perf_counter()
        r.render_hybrid(view, mask)
        r.synchronize()
        rows["call_ms"].append((time.perf_counter() - t0) * 1e3)
        if on:
            s = r.area_light_stats()
            for k in STAGES:
                rows[k].append(getattr(s, k))
    out = {}
    for key, xs in rows.items():
        xs = xs[a.warmup:]
        if xs:
            out[key] = statistics.median(xs)
            out[key + "_spread"] = max(xs) - min(xs)
    if on:
        s = r.area_light_stats()
        out.update(pixels=s.pixels, samples=s.samples, shadow_rays=s.shadow_rays, occluded=s.occluded, emitter_pixels=s.emitter_pixels, emitters=s.emitters,
                   table_builds=s.table_builds, table_ms=s.table_ms, shadow_grays_per_s=s.shadow_rays / (out["shadow_ms"] * 1e-3) / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_lights_timing.json"))
    a = ap.parse_args()
    import rust_renderer_amd as rr

    scene = rr.scenes.cornell_scene(subdivisions=2, tex_size=16)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    view.fxaa_enabled = 1
    times = dict(without_the_bit=timed_calls(a, rr, r, view, rr.HYBRID_FRAME), with_the_bit={})
    for samples in (1, 2, 16):
        for order in (0, 1):
            r.set_option("area_light_order", order)
            r.set_area_light_params(samples=samples)
            times["with_the_bit"][f"order_{order}_{ORDERS[order]}_samples_{samples}"] = timed_calls(a, rr, r, view, rr.HYBRID_FRAME | rr.HYBRID_AREA_LIGHTS)
    r.set_option("area_light_order", 0)
    p = rr.area_light_default_params()
    out = dict(metric="area_lights_timing", scene="cornell", width=a.width, height=a.height, iters=a.iters, times=times,
               params={k: getattr(p, k) for k, _ in p._fields_ if k != "samples"})
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Timing of the ray-traced glossy reflections (UH_HYBRID_GLOSSY) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's
two spheres), warm, through the Python layer: the five stage times of UhGlossyStats (classify + ray generation + closest-hit walk, the
streaming hit shading, the sun rays' any-hit walk, sums + filter, composite) with the pass's totals at 1, 2 and 4 samples, and - in the
same session, on the same scene and at the same sample counts - the stages of UH_HYBRID_RTGI, whose closest-hit kernel shades where the
walk ends: the walk-plus-shade rate of this pass (rays / (trace_ms + shade_ms)) beside k_rtgi_trace's stage (rays / trace_ms). The scene's
materials carry roughness_factor 1, so max_roughness is set to 1.0 and every geometry pixel that faces the camera casts. Each figure is the
median of --iters calls with a wait after each; the spread (max - min) is recorded next to it.

"Without the bit nothing changed" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes (parent and this build, the one that goes first alternating), each measuring the call
without the bit; the parent's run-to-run spread is the yardstick the difference is held against.

  python tools/glossy_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --baseline-lib FILE --rounds 3 --out FILE]
  python tools/glossy_timing.py --plain   (one child's measurement: the call without the bit, as JSON on stdout)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GLOSSY_STAGES = ("trace_ms", "shade_ms", "shadow_ms", "filter_ms", "composite_ms")
RTGI_STAGES = ("trace_ms", "shadow_ms", "filter_ms", "composite_ms")


def setup(a):
    import rust_renderer_amd as rr

    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    view.fxaa_enabled = 1
    return rr, r, view


def timed_calls(a, r, view, mask, stats=None, stages=()):
    rows = dict(call_ms=[], deferred_ms=[], **{k: [] for k in stages})
    for _ in range(a.warmup + a.iters):
        r.synchronize()
        t0 = time.perf_counter()
        r.render_hybrid(view, mask)
        r.synchronize()
        rows["call_ms"].append((time.perf_counter() - t0) * 1e3)
        rows["deferred_ms"].append(r.hybrid_frame_stats().pass_ms[4])
        if stats:
            s = stats()
            for k in stages:
                rows[k].append(getattr(s, k))
    out = {}
    for key, xs in rows.items():
        xs = xs[a.warmup:]
        out[key] = statistics.median(xs)
        out[key + "_spread"] = max(xs) - min(xs)
    return out


def plain(a):
    rr, r, view = setup(a)
    return timed_calls(a, r, view, rr.HYBRID_FRAME)


def measure(a):
    rr, r, view = setup(a)
    out = dict(without_the_bit=timed_calls(a, r, view, rr.HYBRID_FRAME), glossy={}, rtgi={})
    for samples in (1, 2, 4):
        r.set_glossy_params(samples=samples, max_roughness=1.0)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_GLOSSY, r.glossy_stats, GLOSSY_STAGES)
        s = r.glossy_stats()
        row.update(pixels=s.pixels, rays=s.rays, below=s.below, shadow_rays=s.shadow_rays, misses=s.misses,
                   walk_grays_per_s=s.rays / (row["trace_ms"] * 1e-3) / 1e9,
                   walk_plus_shade_grays_per_s=s.rays / ((row["trace_ms"] + row["shade_ms"]) * 1e-3) / 1e9,
                   sun_grays_per_s=s.shadow_rays / (row["shadow_ms"] * 1e-3) / 1e9)
        out["glossy"][f"samples_{samples}"] = row
        r.set_rtgi_params(samples=samples)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_RTGI, r.rtgi_stats, RTGI_STAGES)
        s = r.rtgi_stats()
        row.update(pixels=s.pixels, rays=s.rays, shadow_rays=s.shadow_rays, misses=s.misses,
                   walk_plus_shade_grays_per_s=s.rays / (row["trace_ms"] * 1e-3) / 1e9, sun_grays_per_s=s.shadow_rays / (row["shadow_ms"] * 1e-3) / 1e9)
        out["rtgi"][f"samples_{samples}"] = row
    p = rr.glossy_default_params()
    out["params"] = dict({k: getattr(p, k) for k, _ in p._fields_ if k != "samples"}, max_roughness=1.0)
    return out


def against_parent(a):
    runs = {"parent": [], "this": []}
    cmd = [sys.executable, os.path.abspath(__file__), "--plain", "--width", str(a.width), "--height", str(a.height), "--warmup", str(a.warmup),
           "--iters", str(a.iters)]
    for rnd in range(a.rounds):
        order = (("parent", a.baseline_lib), ("this", None))
        for side, lib in (order if rnd % 2 == 0 else order[::-1]):  # the side that goes first alternates
            env = dict(os.environ)
            env.pop("UTOPIAN_HIP_LIB", None)
            if lib:
                env["UTOPIAN_HIP_LIB"] = os.path.abspath(lib)
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                raise SystemExit(f"child ({side}) failed with status {res.returncode}:\n{res.stderr[-2000:]}")
            runs[side].append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = dict(rounds=a.rounds, runs=runs)
    for key in ("call_ms", "deferred_ms"):
        sides = {s: [x[key] for x in runs[s]] for s in runs}
        out[key] = dict({s: statistics.median(v) for s, v in sides.items()}, **{f"{s}_spread": max(v) - min(v) for s, v in sides.items()})
        out[key]["difference"] = out[key]["this"] - out[key]["parent"]
        out[key]["not_slower_beyond_the_parents_spread"] = out[key]["difference"] <= out[key]["parent_spread"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glossy_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="glossy_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = measure(a)
    out["without_the_bit_against_the_parent_commit"] = against_parent(a) if a.baseline_lib else "not measured (no --baseline-lib)"
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

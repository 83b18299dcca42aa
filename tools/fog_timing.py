"""Timing of the volumetric fog pass (UH_HYBRID_FOG) at 1920 x 1080, warm, through the Python layer, on two scenes: the courtyard of
tests/rtgi_reference.py (the scene of tests/test_gpu_walk_chunks.py: a canopy with an opening, so shafts of light and their shadows) and
the config-1 scene (Sponza-class with the reference's two spheres). With the default params (16 steps, blur_radius 2) and for each of the
trace kernel's three item layouts (option "fog_order" 0, 1, 2: fog.hip): the three stage times of UhFogStats (classify + walk, resolve +
filter, composite), the pass's totals, the walk's rays per second, and - one counted call each - its node visits and triangle tests per
ray. Beside them, in the same session on the same scene, the rtao pass's classify + trace stage at 16 samples (as many rays per pixel) and
at its default 4, with its rays per second: k_rtao_trace is the nearest any-hit item walk. Each figure is the median of --iters calls with
a wait after each; the spread (max - min) is recorded next to it.

"Without the bit nothing changed" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes per scene (parent and this build, the one that goes first alternating), each measuring
the call without the bit; the parent's run-to-run spread is the yardstick the difference is held against.

  python tools/fog_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --baseline-lib FILE --rounds 3 --out FILE]
  python tools/fog_timing.py --plain --scene courtyard|config1   (one child's measurement: the call without the bit, as JSON on stdout)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

SCENES = ("courtyard", "config1")
FOG_STAGES = ("trace_ms", "filter_ms", "composite_ms")


def setup(a, name):
    import rust_renderer_amd as rr

    if name == "courtyard":
        import hybrid_reference as hr
        import rtgi_reference as gi

        scene = gi.courtyard_scene()
        r = rr.Renderer(a.width, a.height)
        hr.upload_recorded(scene, r, True)
    else:
        scene = rr.scenes.scene_for_config(1, with_spheres=True)
        r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    view.fxaa_enabled = 1
    return rr, r, view


def timed_calls(a, r, view, mask, stats=None, stages=()):
    rows = dict(call_ms=[], **{k: [] for k in stages})
    for _ in range(a.warmup + a.iters):
        r.synchronize()
        t0 = time.perf_counter()
        r.render_hybrid(view, mask)
        r.synchronize()
        rows["call_ms"].append((time.perf_counter() - t0) * 1e3)
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
    rr, r, view = setup(a, a.scene)
    return timed_calls(a, r, view, rr.HYBRID_FRAME)


def measure(a, name):
    rr, r, view = setup(a, name)
    out = dict(without_the_bit=timed_calls(a, r, view, rr.HYBRID_FRAME), fog={}, rtao={})
    r.set_fog_params()
    for order in (0, 1, 2):
        r.set_option("fog_order", order)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_FOG, r.fog_stats, FOG_STAGES)
        s = r.fog_stats()
        r.set_option("count_visits", 1)
        r.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_FOG)
        r.set_option("count_visits", 0)
        nodes, tris = r.fog_visits()
        row.update(pixels=s.pixels, rays=s.rays, lit=s.lit, walk_grays_per_s=s.rays / (row["trace_ms"] * 1e-3) / 1e9,
                   node_visits_per_ray=nodes / s.rays, triangle_tests_per_ray=tris / s.rays)
        out["fog"][f"order_{order}"] = row
    r.set_option("fog_order", 2)
    for samples in (16, 4):
        r.set_rtao_params(samples=samples)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_RTAO, r.rtao_stats, ("trace_ms", "filter_ms"))
        s = r.rtao_stats()
        row.update(pixels=s.pixels, rays=s.rays, occluded=s.occluded, walk_grays_per_s=s.rays / (row["trace_ms"] * 1e-3) / 1e9)
        out["rtao"][f"samples_{samples}"] = row
    p = rr.fog_default_params()
    out["params"] = {k: (list(getattr(p, k)) if k in ("albedo", "ambient") else getattr(p, k)) for k, _ in p._fields_}
    return out


def against_parent(a, name):
    runs = {"parent": [], "this": []}
    cmd = [sys.executable, os.path.abspath(__file__), "--plain", "--scene", name, "--width", str(a.width), "--height", str(a.height),
           "--warmup", str(a.warmup), "--iters", str(a.iters)]
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
    sides = {s: [x["call_ms"] for x in runs[s]] for s in runs}
    row = dict({s: statistics.median(v) for s, v in sides.items()}, **{f"{s}_spread": max(v) - min(v) for s, v in sides.items()})
    row["difference"] = row["this"] - row["parent"]
    row["not_slower_beyond_the_parents_spread"] = row["difference"] <= row["parent_spread"]
    out["call_ms"] = row
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
    ap.add_argument("--scene", choices=SCENES, default="config1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fog_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="fog_timing", width=a.width, height=a.height, iters=a.iters, scenes={})
    for name in SCENES:
        row = measure(a, name)
        row["without_the_bit_against_the_parent_commit"] = against_parent(a, name) if a.baseline_lib else "not measured (no --baseline-lib)"
        out["scenes"][name] = row
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

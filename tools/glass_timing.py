"""Timing of the ray-traced glass pass (UH_HYBRID_GLASS) at 1920 x 1080, warm, through the Python layer, on two scenes: rtiow_scene() (its
glass sphere, among the many small ones that are glass too) and the gallery of tests/glass_reference.py. With the default params
(max_events 8): the four stage times of UhGlassStats (classify + first event + the rounds' walks, the rounds' bend kernels, the sun rays'
walk, the composite), the pass's totals, and segments per second over walk + bend. The cost of the rounds that find an empty queue: the
courtyard without glass, where every round is empty, at max_events 1, 8 and 16 - the slope is what one empty round (a walk and a bend
kernel that read a zero and return) costs. Each figure is the median of --iters calls with a wait after each; the spread (max - min)
is recorded next to it.

"Without the bit nothing changed" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes per scene (parent and this build, the one that goes first alternating), each measuring
the all-features call (frame, rtgi, glossy, fog, taa) without the bit; the parent's run-to-run spread is the yardstick the difference is
held against.

  python tools/glass_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --baseline-lib FILE --rounds 3 --out FILE]
  python tools/glass_timing.py --plain --scene rtiow|gallery   (one child's measurement: the call without the bit, as JSON on stdout)"""
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

SCENES = ("rtiow", "gallery")
STAGES = ("trace_ms", "bend_ms", "shadow_ms", "composite_ms")
INTEGERS = ("pixels", "chains", "segments", "events", "tir", "cut", "shadow_rays", "misses")


def setup(a, name):
    import hybrid_reference as hr
    import rust_renderer_amd as rr

    r = rr.Renderer(a.width, a.height)
    if name == "rtiow":
        scene = rr.scenes.rtiow_scene()
        scene.upload(r)
        view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    else:
        import glass_reference as gs
        import rtgi_reference as gi

        scene = gs.gallery_scene() if name == "gallery" else gi.courtyard_scene()
        hr.upload_recorded(scene, r, True)
        view = gs.scene_view(scene, a.width, a.height)
    view.samples_per_frame = view.total_samples = 1
    view.fxaa_enabled = 1
    return rr, r, view


def all_features(rr):
    return rr.HYBRID_FRAME | rr.HYBRID_RTGI | rr.HYBRID_GLOSSY | rr.HYBRID_FOG | rr.HYBRID_TAA


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
    return timed_calls(a, r, view, all_features(rr))


def measure(a, name):
    rr, r, view = setup(a, name)
    out = dict(frame_without_the_bit=timed_calls(a, r, view, rr.HYBRID_FRAME))
    for max_events in (8, 16):
        r.set_glass_params(max_events=max_events)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_GLASS, r.glass_stats, STAGES)
        s = r.glass_stats()
        row.update({k: getattr(s, k) for k in INTEGERS})
        row["segments_per_s_walk_and_bend"] = s.segments / ((row["trace_ms"] + row["bend_ms"]) * 1e-3) if s.segments else 0.0
        row["pass_ms"] = sum(row[k] for k in STAGES)
        out[f"max_events_{max_events}"] = row
    return out


def empty_rounds(a):
    """the courtyard without glass: every round finds an empty queue"""
    rr, r, view = setup(a, "courtyard")
    out = {}
    for max_events in (1, 8, 16):
        r.set_glass_params(max_events=max_events)
        row = timed_calls(a, r, view, rr.HYBRID_FRAME | rr.HYBRID_GLASS, r.glass_stats, STAGES)
        row["pass_ms"] = sum(row[k] for k in STAGES)
        out[f"max_events_{max_events}"] = row
    out["ms_per_empty_round"] = (out["max_events_16"]["trace_ms"] + out["max_events_16"]["bend_ms"] - out["max_events_1"]["trace_ms"] - out["max_events_1"]["bend_ms"]) / 15.0
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
    ap.add_argument("--scene", choices=SCENES, default="gallery")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glass_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="glass_timing", width=a.width, height=a.height, iters=a.iters, scenes={})
    for name in SCENES:
        row = measure(a, name)
        row["all_features_without_the_bit_against_the_parent_commit"] = against_parent(a, name) if a.baseline_lib else "not measured (no --baseline-lib)"
        out["scenes"][name] = row
    out["empty_rounds_on_the_courtyard"] = empty_rounds(a)
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

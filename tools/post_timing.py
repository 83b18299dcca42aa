"""Timing of the HDR display chain (UH_HYBRID_POST) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's two spheres),
warm, through the Python layer: the three stage times of UhPostStats (meter, bloom, tonemap) next to that call's present time
(UhHybridFrameStats) and the whole uh_render_hybrid(HYBRID_FRAME [| HYBRID_POST]) call from its start to the end of a wait behind it,
with and without the bit. Then the two streaming kernels on their own, as bytes moved over hipEvent time: the level-1 kernel (bloom_levels
= 1: the bloom stage is that kernel alone; it reads every frame texel once and writes a quarter as many) and the composite kernel without
bloom (one texel read, one written) and with it (plus the level-1 image). Each figure is the median of --iters calls with a wait after
each; the spread (max - min) is recorded next to it.

"Without the bit nothing changed" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes (parent and this build, the one that goes first alternating), each measuring the call
without the bit.

  python tools/post_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --baseline-lib FILE --rounds 3 --out FILE]
  python tools/post_timing.py --plain   (one child's measurement: the call without the bit, as JSON on stdout)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(a):
    import rust_renderer_amd as rr

    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    view.fxaa_enabled = 1
    return rr, r, view


def timed_calls(a, rr, r, view, mask):
    rows = dict(call_ms=[], deferred_ms=[], present_ms=[], meter_ms=[], bloom_ms=[], tonemap_ms=[])
    post = mask & getattr(rr, "HYBRID_POST", 0)
    for _ in range(a.warmup + a.iters):
        r.synchronize()
        t0 = time.perf_counter()
        r.render_hybrid(view, mask)
        r.synchronize()
        rows["call_ms"].append((time.perf_counter() - t0) * 1e3)
        s = r.hybrid_frame_stats()
        rows["deferred_ms"].append(s.pass_ms[4])
        rows["present_ms"].append(s.pass_ms[6])
        if post:
            p = r.post_stats()
            rows["meter_ms"].append(p.meter_ms), rows["bloom_ms"].append(p.bloom_ms), rows["tonemap_ms"].append(p.tonemap_ms)
    out = {}
    for key, xs in rows.items():
        xs = xs[a.warmup:]
        if xs:
            out[key] = statistics.median(xs)
            out[key + "_spread"] = max(xs) - min(xs)
    return out


def plain(a):
    rr, r, view = setup(a)
    return timed_calls(a, rr, r, view, rr.HYBRID_FRAME)


def measure(a):
    rr, r, view = setup(a)
    out = dict(without_the_bit=timed_calls(a, rr, r, view, rr.HYBRID_FRAME), with_the_bit=timed_calls(a, rr, r, view, rr.HYBRID_FRAME | rr.HYBRID_POST))
    s = r.post_stats()
    out["last_pass"] = dict(exposure=s.exposure, target_exposure=s.target_exposure, average_luminance=s.average_luminance, metered_pixels=s.metered_pixels,
                            bad_pixels=s.bad_pixels, levels=s.levels)
    # the streaming kernels on their own
    pixels = a.width * a.height
    w1, h1 = r.post_level_size(1)
    kernels = {}
    r.set_post_params(bloom_levels=1)
    t = timed_calls(a, rr, r, view, rr.HYBRID_FRAME | rr.HYBRID_POST)
    bytes_moved = 16 * (pixels + w1 * h1)
    kernels["level_1"] = dict(ms=t["bloom_ms"], spread=t["bloom_ms_spread"], bytes=bytes_moved, gb_per_s=bytes_moved / (t["bloom_ms"] * 1e-3) / 1e9)
    bytes_moved = 16 * (2 * pixels + w1 * h1)
    kernels["composite_with_bloom"] = dict(ms=t["tonemap_ms"], spread=t["tonemap_ms_spread"], bytes=bytes_moved, gb_per_s=bytes_moved / (t["tonemap_ms"] * 1e-3) / 1e9)
    for name, op in (("composite_aces", rr.TONEMAP_ACES), ("composite_none", rr.TONEMAP_NONE)):
        r.set_post_params(flags=rr.POST_AUTO_EXPOSURE, tonemap=op)
        t = timed_calls(a, rr, r, view, rr.HYBRID_FRAME | rr.HYBRID_POST)
        bytes_moved = 32 * pixels
        kernels[name] = dict(ms=t["tonemap_ms"], spread=t["tonemap_ms_spread"], bytes=bytes_moved, gb_per_s=bytes_moved / (t["tonemap_ms"] * 1e-3) / 1e9)
    bytes_moved = 16 * pixels
    kernels["meter"] = dict(ms=t["meter_ms"], spread=t["meter_ms_spread"], bytes=bytes_moved, gb_per_s=bytes_moved / (t["meter_ms"] * 1e-3) / 1e9,
                            note="histogram and exposure kernels together")
    out["kernels"] = kernels
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
    for key in ("call_ms", "deferred_ms", "present_ms"):
        sides = {s: [x[key] for x in runs[s]] for s in runs}
        out[key] = dict({s: statistics.median(v) for s, v in sides.items()}, **{f"{s}_spread": max(v) - min(v) for s, v in sides.items()})
        out[key]["difference"] = out[key]["this"] - out[key]["parent"]
        out[key]["within_spread"] = abs(out[key]["difference"]) <= max(out[key]["parent_spread"], out[key]["this_spread"])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="post_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = measure(a)
    out["without_the_bit_against_the_parent_commit"] = against_parent(a) if a.baseline_lib else "not measured (no --baseline-lib)"
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Timing of temporal anti-aliasing (UH_HYBRID_TAA) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's two spheres),
warm, through the Python layer. Per kind of frame - the camera at rest without jitter, and jittered by uh_taa_jitter every call (the
camera grid's matrix compare then fails and the G-buffer cast walks the tree) - UhTaaStats.taa_ms next to that call's deferred and
present times (UhHybridFrameStats), and the whole uh_render_hybrid(HYBRID_FRAME | HYBRID_MOTION [| HYBRID_TAA]) call from its start to
the end of a wait behind it, with and without the bit. Each figure is the median of --iters calls with a wait after each; the spread
(max - min) is recorded next to it.

"Without the bit nothing changed" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes (parent and this build, the one that goes first alternating), each measuring the call
without the bit.

  python tools/taa_timing.py [--width 1920 --height 1080 --warmup 5 --iters 20 --baseline-lib FILE --rounds 3 --out FILE]
  python tools/taa_timing.py --plain   (one child's measurement: the call without the bit, as JSON on stdout)"""
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
    view.fxaa_enabled = 0
    import numpy as np

    p = np.array(view.projection[:], np.float32).reshape(4, 4).T
    v = np.array(view.view[:], np.float32).reshape(4, 4).T
    view.prev_frame_projection_view[:] = rr.camera.to_glam((p @ v).astype(np.float32)).tolist()  # the camera's own: it is at rest
    return rr, r, view


def timed_calls(a, rr, r, view, mask, jitter):
    rows = dict(call_ms=[], deferred_ms=[], present_ms=[], gbuffer_ms=[], taa_ms=[])
    for k in range(a.warmup + a.iters):
        v = rr.Renderer.jitter_view(view, k, a.width, a.height) if jitter else view
        r.synchronize()
        t0 = time.perf_counter()
        r.render_hybrid(v, mask)
        r.synchronize()
        rows["call_ms"].append((time.perf_counter() - t0) * 1e3)
        s = r.hybrid_frame_stats()
        rows["gbuffer_ms"].append(s.pass_ms[1])
        rows["deferred_ms"].append(s.pass_ms[4])
        rows["present_ms"].append(s.pass_ms[6])
        if mask & getattr(rr, "HYBRID_TAA", 0):
            rows["taa_ms"].append(r.taa_stats().taa_ms)
    out = {}
    for key, xs in rows.items():
        xs = xs[a.warmup:]
        if xs:
            out[key] = statistics.median(xs)
            out[key + "_spread"] = max(xs) - min(xs)
    return out


def plain(a):
    rr, r, view = setup(a)
    return timed_calls(a, rr, r, view, rr.HYBRID_FRAME | rr.HYBRID_MOTION, False)


def measure(a):
    rr, r, view = setup(a)
    base = rr.HYBRID_FRAME | rr.HYBRID_MOTION
    out = {}
    for name, jitter in (("camera_at_rest", False), ("jittered", True)):
        out[name] = dict(without_the_bit=timed_calls(a, rr, r, view, base, jitter), with_the_bit=timed_calls(a, rr, r, view, base | rr.HYBRID_TAA, jitter))
    r.set_taa_params(flags=rr.TAA_CLAMP | rr.TAA_MOTION)
    out["jittered"]["with_the_bit_and_TAA_MOTION"] = timed_calls(a, rr, r, view, base | rr.HYBRID_TAA, True)
    s = r.taa_stats()
    out["last_pass"] = dict(history_pixels=s.history_pixels, reset_pixels=s.reset_pixels)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taa_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="taa_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = measure(a)
    out["without_the_bit_against_the_parent_commit"] = against_parent(a) if a.baseline_lib else "not measured (no --baseline-lib)"
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Timing of motion vectors (UH_HYBRID_MOTION) and of the denoiser that follows them (UH_DENOISE_MOTION) at 1920 x 1080 on the config-1
scene (Sponza-class with the reference's two spheres), camera at rest, warm. Three kinds of frame: static, one mesh moved rigidly (the
last mesh, by another small translation every frame), and every mesh's vertices updated (uh_update_mesh_vertices with the vertices it
has: every mesh is `deformed`, every vertex is snapshotted). Per kind: motion_ms and snapshot_ms (UhMotionStats), the G-buffer pass's
pass_ms with and without the bit (UhHybridStats), uh_denoise's input + temporal stage pass_ms[0] with and without the flag. Each figure
is the median of --iters calls with a wait after each.

"Without the bit costs nothing" is a comparison against ANOTHER BUILD: --baseline-lib names the parent commit's libutopian_hip.so. The
tool then runs --rounds pairs of child processes (parent and this build, the one that goes first alternating), each measuring the
G-buffer pass and the temporal stage without the bit, and records every run's medians and the spread of each side next to the difference between the sides.

  python tools/motion_timing.py [--width 1920 --height 1080 --warmup 3 --iters 20 --baseline-lib FILE --rounds 4 --out FILE]
  python tools/motion_timing.py --plain   (one child's measurement: G-buffer and temporal stage without the bit, as JSON on stdout)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(a):
    import rust_renderer_amd as rr

    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    view.rebuild_tlas = 1
    return rr, scene, r, view


def plain(a):
    """the G-buffer cast and the temporal stage without the bit and the flag: what the parent commit has too"""
    rr, scene, r, view = setup(a)
    gbuffer, temporal = [], []
    p = rr.default_denoise_params()
    for _ in range(a.warmup + a.iters):
        r.render_frame(view, rr.PASS_REFERENCE_PT)
        r.render_hybrid(view, rr.HYBRID_GBUFFER)
        r.denoise(view, p)
        gbuffer.append(r.hybrid_stats().pass_ms[0])  # waits
        temporal.append(r.denoise_stats().pass_ms[0])
    return dict(gbuffer_ms=statistics.median(gbuffer[a.warmup:]), temporal_ms=statistics.median(temporal[a.warmup:]))


def measure(a):
    rr, scene, r, view = setup(a)
    meshes = []
    k = 0
    while True:
        try:
            meshes.append(r.read_mesh(k)[0])
        except rr.UtopianError:
            break
        k += 1
    med = lambda xs: statistics.median(xs[a.warmup:])
    old = rr.default_denoise_params()
    new = rr.default_denoise_params()
    new.flags |= rr.DENOISE_MOTION
    out = dict(triangles=scene.num_triangles, meshes=len(meshes), vertices=int(sum(len(m) for m in meshes)), frames={})
    step = [0]

    def static():
        pass

    def rigid():
        step[0] += 1
        r.set_instance_transform(len(meshes) - 1, rr.transform3x4((1.0, 1.0, 1.0), (0.0, 0.001 * step[0], 0.0)))

    def deform_all():
        for i, m in enumerate(meshes):
            if len(m):
                r.update_mesh_vertices(i, m)

    for name, update in (("static", static), ("one_mesh_rigid", rigid), ("whole_scene_vertex_update", deform_all)):
        rows = dict(motion_ms=[], snapshot_ms=[], gbuffer_with_ms=[], gbuffer_without_ms=[], temporal_with_ms=[], temporal_without_ms=[])
        for _ in range(a.warmup + a.iters):
            update()
            r.render_frame(view, rr.PASS_REFERENCE_PT)
            r.render_hybrid(view, rr.HYBRID_GBUFFER | rr.HYBRID_MOTION)
            r.denoise(view, new)
            s = r.motion_stats()  # waits
            rows["motion_ms"].append(s.motion_ms)
            rows["snapshot_ms"].append(s.snapshot_ms)
            rows["gbuffer_with_ms"].append(r.hybrid_stats().pass_ms[0])
            rows["temporal_with_ms"].append(r.denoise_stats().pass_ms[0])
            r.render_hybrid(view, rr.HYBRID_GBUFFER)
            r.denoise(view, old)
            rows["gbuffer_without_ms"].append(r.hybrid_stats().pass_ms[0])
            rows["temporal_without_ms"].append(r.denoise_stats().pass_ms[0])
        out["frames"][name] = dict({k: med(v) for k, v in rows.items()}, meshes_static=s.meshes_static, meshes_rigid=s.meshes_rigid,
                                   meshes_deformed=s.meshes_deformed, meshes_none=s.meshes_none, pixels_with=s.pixels_with,
                                   pixels_without=s.pixels_without)
    return out


def against_parent(a):
    """alternating child processes: the parent commit's library and this build's, the same measurement without the bit"""
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
    for key in ("gbuffer_ms", "temporal_ms"):
        sides = {s: [x[key] for x in runs[s]] for s in runs}
        out[key] = dict({s: statistics.median(v) for s, v in sides.items()}, **{f"{s}_spread": max(v) - min(v) for s, v in sides.items()})
        out[key]["difference"] = out[key]["this"] - out[key]["parent"]
        out[key]["within_spread"] = abs(out[key]["difference"]) <= max(out[key]["parent_spread"], out[key]["this_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_timing.json"))
    a = ap.parse_args()
    if a.plain:
        print(json.dumps(plain(a)))
        return
    out = dict(metric="motion_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = measure(a)
    out["without_the_bit_against_the_parent_commit"] = against_parent(a) if a.baseline_lib else "not measured (no --baseline-lib)"
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

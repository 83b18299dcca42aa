"""Timing of uh_update_isosurface_mesh on BASELINE.json configs[4]'s scene (isosurface_scene(512): the 512^3 field over a ground plane)
at 1920 x 1080 with device_build = 1: what it costs to show the field at another time.

  route A  what the library offered before the verb: a fresh context, the ground, uh_add_isosurface_mesh(t), uh_build_acceleration.
           Only add + build is timed (context creation, the ground and the default texture are not), host clock ending in uh_synchronize.
  route B  uh_update_isosurface_mesh(t) + uh_build_acceleration on a living context, same clock.
  B+frame  route B followed by one path-traced frame (the animated per-frame cost: both grids are rebuilt or bypassed as the library
           decides), same clock.

An untimed pass of each route first; then the routes alternate over the same --times, --rounds times over; medians and the spread
(min .. max) of each. --parent-library PATH runs route A once more, in a process of its own, on another build of the library (the
commit before the verb) and records it as parent_route_a_ms. One JSON document, printed and written to --out.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/isosurface_update_timing.py --rounds 1` for the kernel table.

  python tools/isosurface_update_timing.py [--resolution 512 --width 1920 --height 1080 --times 0.5,1.5,2.5,3.5,4.5 --rounds 3
                                             --parent-library FILE --only-a --out profiles/isosurface_update_timing.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_renderer_amd as rr  # noqa: E402


def new_context(a, scene):
    """a context with everything of the scene except the isosurface"""
    r = rr.Renderer(a.width, a.height)
    r.set_option("device_build", 1)
    r.default_diffuse_map()
    for model, transform in scene.models:
        r.add_model(model, transform)
    return r


def clock(r, fn):
    r.synchronize()
    t0 = time.perf_counter()
    out = fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def route_a(a, scene, t):
    r = new_context(a, scene)

    def work():
        _, tris = r.add_isosurface_mesh(a.resolution, 0.0, 32.0, t)
        r.build_acceleration()
        return tris

    ms, tris = clock(r, work)
    build_ms = r.get_stats().build_ms
    r.close()
    return ms, tris, build_ms


def summary(samples):
    return dict(median=statistics.median(samples), min=min(samples), max=max(samples), spread=max(samples) - min(samples), samples=samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--times", default="0.5,1.5,2.5,3.5,4.5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="another build of the library: route A on it, in a process of its own")
    ap.add_argument("--only-a", action="store_true", help="route A alone (what --parent-library runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    times = [float(x) for x in a.times.split(",")]
    scene = rr.scenes.isosurface_scene(a.resolution)
    doc = dict(metric="isosurface_update", resolution=a.resolution, width=a.width, height=a.height, device_build=1, times=times, rounds=a.rounds,
               library=rr.load_library().uh_version().decode())
    route_a(a, scene, 0.25)  # warm-up
    if a.only_a:
        doc["route_a_ms"] = summary([route_a(a, scene, t)[0] for _ in range(a.rounds) for t in times])
    else:
        live = new_context(a, scene)
        mesh, _ = live.add_isosurface_mesh(a.resolution, 0.0, 32.0, 0.0)
        live.build_acceleration()
        loop = rr.FrameLoop(live, scene.make_view(a.width, a.height))

        def route_b(t, frame):
            def work():
                tris = live.update_isosurface_mesh(mesh, t)
                live.build_acceleration()
                if frame:
                    loop.frame(rr.PASS_ALL)
                return tris

            return clock(live, work)

        route_b(0.25, False), route_b(0.25, True)  # warm-up
        sa, sb, sf, tris, a_build, b_build, extract, scatter = [], [], [], {}, [], [], [], []
        for _ in range(a.rounds):
            for t in times:
                ms, n, build_ms = route_a(a, scene, t)
                sa.append(ms), a_build.append(build_ms)
                ms, nb = route_b(t, False)
                sb.append(ms), b_build.append(live.get_stats().build_ms)
                s = live.isosurface_update_stats()
                extract.append(s.extract_ms), scatter.append(s.scatter_ms)
                assert n == nb == s.triangles, "the two routes extracted different meshes"
                tris[str(t)] = n
                sf.append(route_b(t, True)[0])
        s = live.isosurface_update_stats()
        doc.update(route_a_ms=summary(sa), route_b_ms=summary(sb), route_b_and_frame_ms=summary(sf), triangles=tris,
                   route_a_build_ms=statistics.median(a_build), route_b_build_ms=statistics.median(b_build),
                   extract_ms=statistics.median(extract), scatter_ms=statistics.median(scatter),
                   update_stats=dict(updates=s.updates, triangles=s.triangles, host_geometry_bytes=s.host_geometry_bytes, device_bytes=s.device_bytes),
                   a_over_b=statistics.median(sa) / statistics.median(sb),
                   b_below_a_by_more_than_a_spread=statistics.median(sb) < statistics.median(sa) - (max(sa) - min(sa)))
        live.close()
        if a.parent_library:
            cmd = [sys.executable, os.path.abspath(__file__), "--only-a", "--resolution", str(a.resolution), "--width", str(a.width), "--height", str(a.height),
                   "--times", a.times, "--rounds", str(a.rounds)]
            out = subprocess.run(cmd, env=dict(os.environ, UTOPIAN_HIP_LIB=os.path.abspath(a.parent_library)), capture_output=True, text=True, check=True, timeout=900)
            parent = json.loads(out.stdout.strip().splitlines()[-1])
            doc.update(parent_route_a_ms=parent["route_a_ms"], parent_library=parent["library"])
    line = json.dumps(doc)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

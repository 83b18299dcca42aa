"""Timing of uh_update_mesh_vertices on BASELINE.json configs[1]'s scene (scene_for_config(1)) at 1920 x 1080 with device_build = 1: its
largest mesh displaced along its normals by a travelling sine, what it costs to show the next phase.

  route A  what the library offered before the verb: a fresh context, every uh_add_mesh (the displaced mesh among them),
           uh_build_acceleration. Context creation and the textures are not timed; host clock ending in uh_synchronize.
  route B  uh_update_mesh_vertices(UH_VERTICES_DEVICE) + uh_refit_acceleration on a living context, same clock. The phases' vertices
           are in device buffers before the clock starts, as a simulation's own kernels would leave them.
  route C  the same update + uh_build_acceleration.
  B+frame  route B followed by one path-traced frame.

An untimed pass of each route first; then the routes alternate over the same --phases, --rounds times over; medians and the spread
(min .. max) of each, the two hipEvent figures of uh_get_mesh_update_stats, and k_deform_gather's traffic over its time as a fraction
of 8 TB/s: 260 bytes per triangle of the moved mesh (12 of indices, 3 x 48 of vertices, 4 of the key, 36 + 64 written) and the 4
bytes of the key for every other packet. --parent-library PATH runs route A once more, in a process of its own, on another build of
the library (the commit before the verb) and records it as parent_route_a_ms. One JSON document, printed and written to --out.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/mesh_deform_timing.py --rounds 1` for the kernel table.

  python tools/mesh_deform_timing.py [--width 1920 --height 1080 --phases 5 --rounds 3 --parent-library FILE --only-a
                                      --out profiles/mesh_deform_timing.json]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_renderer_amd as rr  # noqa: E402
from rust_renderer_amd.api import compose3x4  # noqa: E402

HBM_PEAK = 8.0e12


def largest_mesh(scene):
    """(model, mesh) positions of the mesh with the most triangles, and its index in a context the scene was uploaded to"""
    best, flat = None, 0
    for mi, (model, _) in enumerate(scene.models):
        for k, mesh in enumerate(model.meshes):
            if best is None or len(mesh.indices) > best[3]:
                best = (mi, k, flat, len(mesh.indices))
            flat += 1
    return best[:3]


def displaced(base, phase):
    v = base.copy()
    p, n = base["pos"][:, :3].astype(np.float64), base["normal"][:, :3].astype(np.float64)
    extent = float(np.ptp(p, axis=0).max()) or 1.0
    wave = 0.02 * extent * np.sin(12.0 * (p[:, 0] + 0.7 * p[:, 1] + 0.4 * p[:, 2]) / extent + 0.8 * phase)
    v["pos"][:, :3] = (p + wave[:, None] * n).astype(np.float32)
    return v


def with_mesh(scene, where, vertices):
    models = list(scene.models)
    model, transform = models[where[0]]
    meshes = list(model.meshes)
    meshes[where[1]] = dataclasses.replace(meshes[where[1]], vertices=vertices)
    models[where[0]] = (dataclasses.replace(model, meshes=meshes), transform)
    return models


def new_context(a):
    r = rr.Renderer(a.width, a.height)
    r.set_option("device_build", 1)
    r.default_diffuse_map()
    return r


def clock(r, fn):
    r.synchronize()
    t0 = time.perf_counter()
    fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def mesh_calls(r, models):
    """the scene's textures into the context and the arguments of its add_mesh calls (Renderer.add_model in its two halves)"""
    calls = []
    for model, transform in models:
        tex = {}
        for mesh in model.meshes:
            mat = mesh.material_struct()
            if mesh.texture is None:
                mat.diffuse_map = r.default_diffuse_map()
            else:
                if mesh.texture not in tex:
                    tex[mesh.texture] = r.add_texture(model.textures[mesh.texture])
                mat.diffuse_map = tex[mesh.texture]
            calls.append((mesh.vertices, mesh.indices, mat, mesh.transform if transform is None else compose3x4(transform, mesh.transform)))
    return calls


def route_a(a, models):
    r = new_context(a)
    calls = mesh_calls(r, models)

    def work():
        for call in calls:
            r.add_mesh(*call)
        r.build_acceleration()

    ms = clock(r, work)
    r.close()
    return ms


def summary(samples):
    return dict(median=statistics.median(samples), min=min(samples), max=max(samples), spread=max(samples) - min(samples), samples=samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--phases", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="another build of the library: route A on it, in a process of its own")
    ap.add_argument("--only-a", action="store_true", help="route A alone (what --parent-library runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scene = rr.scenes.scene_for_config(1)
    where = largest_mesh(scene)
    base = scene.models[where[0]][0].meshes[where[1]].vertices
    phases = [displaced(base, k + 1) for k in range(a.phases)]
    doc = dict(metric="mesh_deform", config=1, width=a.width, height=a.height, device_build=1, phases=a.phases, rounds=a.rounds,
               scene_triangles=scene.num_triangles, mesh_vertices=len(base), mesh_triangles=len(scene.models[where[0]][0].meshes[where[1]].indices) // 3,
               library=rr.load_library().uh_version().decode())
    route_a(a, with_mesh(scene, where, phases[0]))  # warm-up
    if a.only_a:
        doc["route_a_ms"] = summary([route_a(a, with_mesh(scene, where, v)) for _ in range(a.rounds) for v in phases])
    else:
        live = new_context(a)
        for call in mesh_calls(live, scene.models):
            live.add_mesh(*call)
        live.build_acceleration()
        mesh = where[2]
        assert len(live.read_mesh(mesh)[0]) == len(base)
        hip = C.CDLL("libamdhip64.so.7")  # the runtime the library bound
        hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
        buffers = []
        for v in phases:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), v.nbytes) == 0 and hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0
            buffers.append(p.value)
        assert hip.hipDeviceSynchronize() == 0
        loop = rr.FrameLoop(live, scene.make_view(a.width, a.height))

        def route(k, way, frame=False):
            def work():
                live.update_mesh_vertices(mesh, device_ptr=buffers[k], count=len(base))
                live.rebuild_tlas() if way == "refit" else live.build_acceleration()
                if frame:
                    loop.frame(rr.PASS_ALL)

            return clock(live, work)

        route(0, "refit"), route(0, "build"), route(0, "refit", True)  # warm-up
        sa, sb, sc, sf, gather, refit = [], [], [], [], [], []
        for _ in range(a.rounds):
            for k, v in enumerate(phases):
                sa.append(route_a(a, with_mesh(scene, where, v)))
                sb.append(route(k, "refit"))
                s = live.mesh_update_stats()
                gather.append(s.gather_ms), refit.append(s.refit_ms)
                sc.append(route(k, "build"))
                sf.append(route(k, "refit", True))
        s = live.mesh_update_stats()
        gather_bytes = 260 * s.triangles + 4 * (scene.num_triangles - s.triangles)
        doc.update(route_a_ms=summary(sa), route_b_ms=summary(sb), route_c_ms=summary(sc), route_b_and_frame_ms=summary(sf),
                   gather_ms=summary(gather), refit_ms=summary(refit), gather_bytes=gather_bytes,
                   gather_fraction_of_hbm_peak=gather_bytes / (statistics.median(gather) * 1e-3) / HBM_PEAK,
                   update_stats=dict(updates=s.updates, triangles=s.triangles, host_geometry_bytes=s.host_geometry_bytes, device_bytes=s.device_bytes),
                   a_over_b=statistics.median(sa) / statistics.median(sb),
                   b_below_a_by_more_than_a_spread=statistics.median(sb) < statistics.median(sa) - (max(sa) - min(sa)))
        live.close()
        for p in buffers:
            hip.hipFree(p)
        if a.parent_library:
            cmd = [sys.executable, os.path.abspath(__file__), "--only-a", "--width", str(a.width), "--height", str(a.height), "--phases", str(a.phases),
                   "--rounds", str(a.rounds)]
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

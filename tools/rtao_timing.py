"""Timing of ray-traced ambient occlusion (UH_HYBRID_RTAO) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's two
spheres), camera at rest, warm. For samples 1, 4 and 16, at radius 1.0 and at a tenth of the scene's extent (the longest side of its
bounding box), and for each layout of the trace kernel's work ("rtao_order" 0, 1, 2: rtao.hip): the hipEvent ms of classify + trace and of
the resolve / filter (UhRtaoStats), and the AO rays' rate; per setting also the node visits and triangle tests per ray (one pass with
"count_visits" on, not among the timed ones). In the SAME run, as the yardsticks: rt_shadows (one coherent ray per pixel)
with its ms and rate, and the k_hybrid_ssao pass the rtao pass replaces (a frame without the bit). Each figure is the median of --iters
calls with a wait after each. Beside them the compiler's figures for the kernels of csrc/rtao.hip as built for gfx950. Writes one JSON
object to --out (default profiles/rtao_timing.json) and prints it. --resources-only skips the GPU part (a machine without one).

  python tools/rtao_timing.py [--width 1920 --height 1080 --warmup 3 --iters 20 --samples 1,4,16 --out FILE --resources-only]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDERS = {0: "ray_items_samples_of_a_pixel_together", 1: "ray_items_one_sample_of_consecutive_pixels", 2: "pixel_items_lane_walks_its_samples"}


def resources():
    """per kernel of rtao.hip: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD"""
    csrc = os.path.join(ROOT, "rust-renderer_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
           "-I", csrc, "--cuda-device-only", "-c", os.path.join(csrc, "rtao.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = {}, None
    names = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "waves_per_simd",
             "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in out.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip().split("(")[0]
            rows[cur] = {}
        elif cur:
            rows[cur][names[k]] = int(v)
    return rows


def scene_extent(scene):
    """the longest side of the world-space bounding box of the scene's vertices"""
    import rust_renderer_amd as rr

    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for model, transform in scene.models:
        for mesh in model.meshes:
            w = np.asarray(mesh.transform if transform is None else rr.api.compose3x4(transform, mesh.transform), np.float64).reshape(3, 4)
            p = mesh.vertices["pos"][:, :3].astype(np.float64) @ w[:, :3].T + w[:, 3]
            lo, hi = np.minimum(lo, p.min(axis=0)), np.maximum(hi, p.max(axis=0))
    return float((hi - lo).max())


def measure(a):
    import rust_renderer_amd as rr

    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    med = lambda xs: statistics.median(xs[a.warmup:])
    mrays = lambda rays, ms: rays / ms / 1e3 if ms > 0 else 0.0
    # the frame without the bit: ssao.frag's pass, and rt_shadows
    ssao, shadows = [], []
    for _ in range(a.warmup + a.iters):
        r.render_hybrid(view, rr.HYBRID_FRAME)
        s = r.hybrid_frame_stats()  # waits
        ssao.append(s.pass_ms[3])
        shadows.append(s.pass_ms[0])
    shadow_rays = int(r.hybrid_stats().rays[1])
    out = dict(triangles=scene.num_triangles, scene_extent=scene_extent(scene), ssao_ms=med(ssao), rt_shadows_ms=med(shadows), rt_shadows_rays=shadow_rays,
               rt_shadows_mrays_per_s=mrays(shadow_rays, med(shadows)), settings=[])
    for radius_name, radius in (("1.0", 1.0), ("extent / 10", out["scene_extent"] / 10.0)):
        for samples in a.samples:
            r.set_rtao_params(samples=samples, radius=radius)
            row = dict(samples=samples, radius=radius, radius_is=radius_name, orders={})
            for order, name in ORDERS.items():
                r.set_option("rtao_order", order)
                trace, filt, shadows = [], [], []
                for _ in range(a.warmup + a.iters):
                    r.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_RTAO)
                    s = r.rtao_stats()  # waits
                    trace.append(s.trace_ms)
                    filt.append(s.filter_ms)
                    shadows.append(r.hybrid_frame_stats().pass_ms[0])
                row["orders"][name] = dict(order=order, trace_ms=med(trace), filter_ms=med(filt), mrays_per_s=mrays(s.rays, med(trace)),
                                           rt_shadows_ms=med(shadows), rt_shadows_mrays_per_s=mrays(shadow_rays, med(shadows)))
                row.update(pixels=int(s.pixels), rays=int(s.rays), occluded=int(s.occluded))
            # one more pass with the walks counted (another instantiation of the kernel: not among the timed ones)
            r.set_option("rtao_order", 0)
            r.set_option("count_visits", 1)
            r.render_hybrid(view, rr.HYBRID_FRAME | rr.HYBRID_RTAO)
            nodes, tris = r.rtao_visits()
            r.set_option("count_visits", 0)
            row.update(node_visits_per_ray=nodes / max(1, row["rays"]), triangle_tests_per_ray=tris / max(1, row["rays"]))
            out["settings"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=lambda s: [int(x) for x in s.split(",")], default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtao_timing.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    out = dict(metric="rtao_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = "not measured" if a.resources_only else measure(a)
    out["kernels"] = resources()
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

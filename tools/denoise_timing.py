"""Timing of the denoiser (uh_denoise) at 1920 x 1080 on the config-1 scene (Sponza-class with the reference's two spheres), camera at
rest, warm: one path-traced frame of one sample (UhStats.last_frame_ms), one hybrid G-buffer cast and one uh_denoise at the default
params - the hipEvent ms of its four stages (input + temporal, variance estimate, the a-trous levels, output) -, each the median of
--iters calls with a wait after each. Beside them the compiler's figures for the kernels of csrc/denoise.hip as built for gfx950:
registers, scratch, LDS and occupancy. Writes one JSON object to --out (default profiles/denoise_timing.json) and prints it.
--resources-only skips the GPU part (a machine without one): the times are then "not measured".

  python tools/denoise_timing.py [--width 1920 --height 1080 --warmup 3 --iters 20 --out FILE --resources-only]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("input_temporal", "variance", "atrous", "output")


def resources():
    """per kernel of denoise.hip: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD"""
    csrc = os.path.join(ROOT, "rust-renderer_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
           "-I", csrc, "--cuda-device-only", "-c", os.path.join(csrc, "denoise.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
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


def measure(a):
    import rust_renderer_amd as rr

    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    r = scene.upload(rr.Renderer(a.width, a.height))
    view = scene.make_view(a.width, a.height, shadows_enabled=0, ibl_enabled=0, cubemap_enabled=0)
    view.samples_per_frame = view.total_samples = 1
    loop = rr.FrameLoop(r, view)
    loop.end_frame()  # prev_frame_projection_view = this camera's projection * view: a camera at rest
    frame, gbuffer, stages = [], [], []
    for k in range(a.warmup + a.iters):
        view.time = 0.125 * k
        r.render_frame(view, rr.PASS_REFERENCE_PT)
        frame.append(r.get_stats().last_frame_ms)  # waits
        r.render_hybrid(view, rr.HYBRID_GBUFFER)
        gbuffer.append(r.hybrid_frame_stats().pass_ms[1])
        r.denoise(view)
        s = r.denoise_stats()
        stages.append(list(s.pass_ms))
    med = lambda xs: statistics.median(xs[a.warmup:])
    per = {f"{name}_ms": med([s[k] for s in stages]) for k, name in enumerate(STAGES)}
    p = rr.default_denoise_params()
    return dict(frame_ms=med(frame), gbuffer_cast_ms=med(gbuffer), **per, denoise_ms=sum(per.values()), geometry_pixels=s.geometry_pixels,
                history_pixels=s.history_pixels, iterations=p.iterations, triangles=scene.num_triangles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_timing.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    out = dict(metric="denoise_timing", config=1, width=a.width, height=a.height, iters=a.iters)
    out["times"] = "not measured" if a.resources_only else measure(a)
    out["kernels"] = resources()
    text = json.dumps(out, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The lone frame with a wait, which bench.py does not cover: config 1's scene at 1920 x 1080, one frame per call and uh_synchronize
after each, so that every frame finds the GPU idle and takes the fused path (csrc/frame_plan.h plan_sample). Prints one JSON line:
wall-clock ms per call over 64 calls behind 8 warm-up calls, and - from four more calls with option time_kernels - the closest-hit
brackets per frame, which say that the fused kernel ran: 1 (k_path_fused's; bounce 0 goes through the camera grid, another kind),
where the wavefront of launches would show one per bounce. UTOPIAN_HIP_LIB names another build of the library
(profiles/frame_loop_ab.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_renderer_amd as rr

W, H, CALLS = 1920, 1080, 64
scene = rr.scenes.scene_for_config(1, tex_size=1024, detail=1.0)
r = scene.upload(rr.Renderer(W, H, device=0))
loop = rr.FrameLoop(r, scene.make_view(W, H))
for _ in range(8):
    loop.frame(rr.PASS_REFERENCE_PT)
    r.synchronize()
t0 = time.perf_counter()
for _ in range(CALLS):
    loop.frame(rr.PASS_REFERENCE_PT)
    r.synchronize()
ms = (time.perf_counter() - t0) / CALLS * 1e3
r.set_option("time_kernels", 1)
r.reset_stats()
for _ in range(4):
    loop.frame(rr.PASS_REFERENCE_PT)
    r.synchronize()
s = r.get_stats()
print(json.dumps({"lone_frame_ms": ms, "closest_launches_per_frame": s.trace_closest_launches / 4.0}))

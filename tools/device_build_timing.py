"""Option "device_build": build time and traversal quality of the Morton-order tree against the host SAH tree."""
import os
import sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_renderer_amd as rr
W, H = 1920, 1080
for cfg in (1, 3):
    scene = rr.scenes.scene_for_config(cfg, tex_size=64)
    for dev in (0, 1, 2):
        r = rr.Renderer(W, H)
        r.set_option("device_build", dev)
        t0 = time.perf_counter(); scene.upload(r); first = (time.perf_counter() - t0) * 1e3
        s = r.get_stats()
        t0 = time.perf_counter(); r.set_instance_transform(0, rr.identity3x4()); r.initialize_raytracing(); again = (time.perf_counter() - t0) * 1e3
        r.set_option("count_visits", 1)
        loop = rr.FrameLoop(r, scene.make_view(W, H, use_ris_light_sampling=0))
        loop.frame(rr.PASS_REFERENCE_PT)
        c = r.get_stats()
        cl = c.rays[0] + c.rays[1]; sh = c.rays[2] + c.rays[3]
        r.set_option("count_visits", 0)
        r.reset_accumulation(); r.reset_stats()
        loop = rr.FrameLoop(r, scene.make_view(W, H, use_ris_light_sampling=0))
        loop.frames(8, rr.PASS_REFERENCE_PT); r.synchronize()
        t0 = time.perf_counter(); loop.frames(32, rr.PASS_REFERENCE_PT); r.synchronize(); ms = (time.perf_counter() - t0) * 1e3 / 32
        print("config %d %-6s tris %8d nodes %8d | upload+build %7.1f ms (build_ms %6.1f) rebuild %6.1f ms | closest nodes/ray %.2f tris/ray %.2f shadow %.2f / %.2f | %.3f ms/frame" % (
            cfg, ("host", "PLOC", "radix")[dev], s.bvh_triangles, s.bvh_nodes, first, s.build_ms, again, c.nodes_visited / cl, c.tris_tested / cl,
            c.shadow_nodes_visited / max(sh, 1), c.shadow_tris_tested / max(sh, 1), ms), flush=True)

"""The enqueue follows the plan of a sample (csrc/frame_plan.h plan_sample, held on the CPU by tests/cpp/frame_plan_check.cpp; the
enqueue is csrc/frame_loop.hip enqueue_path_trace), seen through a figure the library already reports: with option "time_kernels"
every bracket of kind 0 around a closest-hit launch counts into UhStats.trace_closest_launches."""
import pytest

import rust_renderer_amd as rr

pytestmark = pytest.mark.gpu

W, H, BOUNCES, FRAMES = 64, 48, 3, 3


# What the plan implies for one frame of 3 bounces, one sample, sun on, lights off, no grid (so bounce 0 is a tree walk, kind 0, and
# not the camera grid's kind 3), one frame per call with a wait behind it:
#  fused_bounces = -1: fused (a lone frame, 2 <= 3 <= 64 bounces, fused_always) - the wavefront runs bounce 0 alone, one bracket, and
#                      k_path_fused has one of its own: 2
#  fused_bounces =  0: not fused - the wavefront runs every bounce, one bracket each: 3
# (the sun rays' brackets are kind 1, the shading kernels' kind 2; nothing else of the frame is kind 0)
@pytest.mark.parametrize("fused_bounces,per_frame", [(-1, 1 + 1), (0, BOUNCES)])
def test_closest_hit_brackets_per_frame_are_the_plans(fused_bounces, per_frame):
    scene = rr.scenes.cornell_scene(subdivisions=2, tex_size=16)
    r = scene.upload(rr.Renderer(W, H))
    for name, value in (("time_kernels", 1), ("sun_grid", 0), ("camera_grid", 0), ("fused_bounces", fused_bounces)):
        r.set_option(name, value)
    loop = rr.FrameLoop(r, scene.make_view(W, H, num_bounces=BOUNCES, samples_per_frame=1, sun_shadow_enabled=1, lights_enabled=0))
    seen = []
    for _ in range(FRAMES):
        before = r.get_stats().trace_closest_launches
        loop.frame(rr.PASS_REFERENCE_PT)
        r.synchronize()
        seen.append(r.get_stats().trace_closest_launches - before)
    print(f"fused_bounces = {fused_bounces}: kind-0 brackets per frame {seen}, expected {per_frame}")
    assert seen == [per_frame] * FRAMES

"""GPU: uh_denoise with UH_DENOISE_MOTION over the motion image of UH_HYBRID_MOTION: on a static scene it is the old path bit for bit; the
device against the restatement of tests/denoise_motion_reference.py while the panel moves, deforms and the isosurface changes topology;
the history follows a moving panel, is lost only where there is no correspondence, and what moves is denoised."""
import numpy as np
import pytest

import denoise_motion_reference as dmr
import rust_renderer_amd as rr
from hybrid_util import bits
from motion_util import ISO, PANEL, PANEL_WORLD, SIZES, MotionRig, mapped, rot
from test_gpu_denoise import EXPF_COLOUR_HELD, EXPF_HELD, params, rel_diff

pytestmark = pytest.mark.gpu

F = np.float32
OLD = rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE
NEW = OLD | rr.DENOISE_MOTION
STEP = 0.1  # the panel's approach per frame: five times the default plane tolerance (0.005 of the view depth 4)


def approach(k):
    return rr.transform3x4((1.0, 1.0, 1.0), (0.0, 1.4, STEP * k))


# ---- 6. static equals the old path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_static_scene_equals_the_old_path_bit_for_bit(size):
    a, b = MotionRig(size), MotionRig(size)
    for call in range(3):
        for r, motion, flags in ((a, False, OLD), (b, True, NEW)):
            v = r.shoot(r.view(0.2 * call), motion=motion)
            r.denoise(v, params(flags=flags))
        ia, ib = a.images(), b.images()
        for k in ia:
            assert np.array_equal(ia[k].view(np.uint8), ib[k].view(np.uint8)), (call, k)
        sa, sb = a.gpu.denoise_stats(), b.gpu.denoise_stats()
        assert (sa.geometry_pixels, sa.history_pixels) == (sb.geometry_pixels, sb.history_pixels)
    assert sb.history_pixels > 0 and (ib["history"] == 3).any()


# ---- 7. the device against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_device_equals_the_restatement_while_the_scene_moves(size):
    r = MotionRig(size)
    p = params(flags=NEW, iterations=3)
    ref, pd = dmr.MotionDenoiser(), dmr.params_of(p)
    moved = rr.transform3x4((1.0, 1.0, 1.0), (0.3, 1.45, 0.2), rot(0.0, 0.08, 0.03))
    bent = mapped(r.panel_v, np.concatenate([np.eye(3), [[0.0], [0.0], [0.0]]], axis=1))
    bent["pos"][:, 2] += F(0.15) * np.sin(bent["pos"][:, 0] * F(1.5)).astype(np.float32)
    worst = worst_colour = 0.0
    for call in range(4):
        if call == 1:
            r.gpu.set_instance_transform(PANEL, moved)       # rigid
        elif call == 2:
            r.gpu.update_mesh_vertices(PANEL, bent)          # deformed
        elif call == 3:
            r.gpu.update_isosurface_mesh(ISO, 3.0)           # topology
            r.gpu.build_acceleration()
        v = r.shoot(r.view(0.1 * call))
        r.denoise(v, p)
        inputs = r.inputs()
        want, im = ref(*inputs, v, pd), r.images()
        geo, kept = want["geometry"], want["kept"]
        s, ms = r.gpu.denoise_stats(), r.gpu.motion_stats()
        assert (ms.meshes_rigid, ms.meshes_deformed, ms.meshes_none) == (call == 1, call == 2, call == 3)
        assert np.array_equal(bits(im["history"]), bits(want["history"])), "history length: bit for bit"
        assert (s.geometry_pixels, s.history_pixels) == (geo.sum(), kept.sum())
        assert np.array_equal(bits(im["input"]), bits(want["input"]))
        mesh = inputs[4][..., 3]
        if call:
            on_panel = kept[geo & (mesh == PANEL)]
            print(f"call {call}: history kept on {kept.sum() / geo.sum():.3f} of {geo.sum()} geometry pixels, on {on_panel.mean():.3f} of the panel's")
            assert kept.any() and not kept[geo].all(), "kept and dropped histories both occur"
            if call < 3:
                assert on_panel.mean() >= 0.5, "the moving panel keeps its history"
            else:
                assert not kept[geo & (mesh == ISO)].any() and (geo & (mesh == ISO)).any(), "no correspondence: no history"
        else:
            assert not kept.any()
        acc_n = r.gpu.read_accumulation()[..., :3] / F(v.total_samples)
        scale = np.maximum(np.abs(want["temporal"][..., :3]), np.abs(acc_n)).astype(np.float64)
        assert (np.abs(im["temporal"][..., :3].astype(np.float64) - want["temporal"][..., :3]) <= 4 * (call + 1) * 2.0 ** -23 * scale).all()
        assert np.abs(im["output"].astype(int) - want["output"].astype(int)).max() <= 1, "the 8-bit image within 1 LSB"
        worst = max(worst, rel_diff(im["variance"], want["variance"]))
        worst_colour = max(worst_colour, rel_diff(im["color"][..., :3], want["color"][..., :3]))
    worst = max(worst, worst_colour)
    print(f"expf: largest relative difference of colour {worst_colour:.3e}, of colour and variance {worst:.3e}")
    assert worst <= EXPF_HELD and worst_colour <= EXPF_COLOUR_HELD


# ---- 8. the history follows the panel --------------------------------------------------------------------------------------------
def taps_on_the_panel(motion, prev_mesh, prev_pv, size):
    """panel-independent part: for every pixel, whether the four bilinear taps of the motion texel's reprojection through prev_pv all lie
    in the frame and on the panel in the previous frame's pbr.a (float32, as the stage forms them)"""
    W, H = size
    pv = np.array(prev_pv, np.float32)
    PP = motion[..., :3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        h = [((pv[r] * PP[:, 0] + pv[4 + r] * PP[:, 1]) + pv[8 + r] * PP[:, 2]) + pv[12 + r] * F(1.0) for r in range(4)]
        fx = ((h[0] / h[3]) * F(0.5) + F(0.5)) * F(W) - F(0.5)
        fy = (F(1.0) - ((h[1] / h[3]) * F(0.5) + F(0.5))) * F(H) - F(0.5)
        ok = (h[3] > 0) & np.isfinite(fx) & np.isfinite(fy)
        ix, iy = np.floor(np.where(ok, fx, 0)).astype(np.int64), np.floor(np.where(ok, fy, 0)).astype(np.int64)
    prev = prev_mesh.reshape(-1)
    for dx in (0, 1):
        for dy in (0, 1):
            tx, ty = ix + dx, iy + dy
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            ok &= inside & (prev[np.clip(ty, 0, H - 1) * W + np.clip(tx, 0, W - 1)] == PANEL)
    return ok.reshape(H, W)


@pytest.mark.parametrize("size", SIZES)
def test_history_follows_the_panel(size):
    with_flag, without = MotionRig(size), MotionRig(size)
    prev_mesh = None
    for k in range(1, 6):
        for r, flags in ((with_flag, NEW), (without, OLD)):
            r.gpu.set_instance_transform(PANEL, approach(k))
            v = r.shoot(r.view())
            if r is with_flag:
                prev_pv = r.prev_pv  # projection * view of the previous call
            r.denoise(v, params(flags=flags, max_history=32))
        motion = with_flag.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE)
        mesh = with_flag.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3]
        geo = with_flag.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
        panel = geo & (mesh == PANEL)
        h_with, h_without = with_flag.gpu.read_denoised(rr.DENOISE_HISTORY), without.gpu.read_denoised(rr.DENOISE_HISTORY)
        if k == 1:
            assert (h_with[panel] == 1).all() and (h_without[panel] == 1).all()
        else:
            q = panel & (motion[..., 3] == 1) & taps_on_the_panel(motion, prev_mesh, prev_pv, size)
            print(f"frame {k}: {q.sum()} of {panel.sum()} panel pixels qualify")
            assert 2 * q.sum() >= panel.sum(), "against a vacuous pass: at least half of the panel's pixels qualify"
            assert (h_with[q] == k).all(), "the history follows the panel"
            assert (h_without[q] == 1).all(), "without the flag and without a reset the moved panel has no history"
        prev_mesh = mesh


# ---- 9. no correspondence: a local loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_a_topology_change_loses_the_history_of_its_own_pixels_only(size):
    r = MotionRig(size)
    p = params(flags=NEW)
    for _ in range(3):
        r.denoise(r.shoot(r.view()), p)
    prev_mesh = r.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3]
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    assert (r.gpu.read_denoised(rr.DENOISE_HISTORY)[geo] == 3).all()
    r.gpu.update_isosurface_mesh(ISO, 3.0)
    r.gpu.build_acceleration()
    r.denoise(r.shoot(r.view()), p)
    mesh = r.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3]
    geo = r.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0
    h = r.gpu.read_denoised(rr.DENOISE_HISTORY)
    iso = geo & (mesh == ISO)
    kept = geo & ~iso & (prev_mesh == mesh)  # the camera is at rest: a pixel reprojects onto itself
    assert iso.sum() >= 4 and (h[iso] == 1).all(), "the isosurface's pixels start again"
    for m in (0, PANEL):
        assert (kept & (mesh == m)).any() and (h[kept & (mesh == m)] == 4).all(), "the others keep their history"
    assert (h[kept] == 4).all() and (h[geo & ~kept] == 1).all()
    assert r.gpu.denoise_stats().history_pixels == kept.sum()
    assert r.gpu.motion_stats().pixels_without == iso.sum()


# ---- 10. it denoises what moves ----------------------------------------------------------------------------------------------------
def test_it_denoises_what_moves():
    size, frames, spp = (67, 45), 8, 2048  # 2,048 samples: the comparison is the same against 1,024 (asserted below)
    truth = MotionRig(size)
    truth.gpu.set_instance_transform(PANEL, approach(frames))
    converged = []
    for n in (spp // 2, spp):
        truth.shoot(truth.view(), spp=n, gbuffer=False)
        converged.append(truth.gpu.read_accumulation()[..., :3].astype(np.float64) / n)
    follow, reset = MotionRig(size), MotionRig(size)
    for k in range(1, frames + 1):
        for r in (follow, reset):
            r.gpu.set_instance_transform(PANEL, approach(k))
            v = r.shoot(r.view())
            if r is reset:
                r.reset()  # the caller's only alternative without motion vectors
            r.denoise(v, params(flags=NEW if r is follow else OLD))
    panel = (follow.gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] != 0) & (follow.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3] == PANEL)
    assert panel.sum() > 100
    assert np.array_equal(bits(follow.gpu.read_accumulation()), bits(reset.gpu.read_accumulation())), "both saw the same samples"
    for want in converged:
        mae = [float(np.abs(r.gpu.read_denoised(rr.DENOISE_COLOR)[..., :3].astype(np.float64) - want)[panel].mean()) for r in (follow, reset)]
        noisy = float(np.abs(follow.gpu.read_accumulation()[..., :3].astype(np.float64) - want)[panel].mean())
        print(f"mean absolute error on {panel.sum()} panel pixels: 1 spp {noisy:.5g}, reset every call {mae[1]:.5g}, with motion vectors {mae[0]:.5g}")
        assert mae[0] < mae[1]
    assert (follow.gpu.read_denoised(rr.DENOISE_HISTORY)[panel] > 1).mean() > 0.5

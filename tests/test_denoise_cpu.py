"""CPU: the numpy restatement of uh_denoise (tests/denoise_reference.py) held to known answers on synthetic arrays - the six cases of
DESIGN.md section 2, "Denoiser". test_gpu_denoise.py runs cases 1, 4, 5 and 6 on the device and holds the device to the restatement."""
import numpy as np
import pytest

import denoise_reference as dr
import rust_renderer_amd as rr
from hybrid_util import cast_planes, plane_view

F = np.float32
W, H = 40, 24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def projection_view(view):
    """projection * view, column-major, as a caller hands it over in prev_frame_projection_view"""
    m = lambda a: np.array(a[:], np.float64).reshape(4, 4).T
    return tuple((m(view.projection) @ m(view.view)).T.reshape(-1).astype(np.float32))


@pytest.fixture(scope="module")
def floor_frame():
    """a camera above a floor, the upper rows sky: view, position, normal, albedo, pbr"""
    view = plane_view((0.0, 1.5, 4.0), (0.0, 0.5, 0.0), W, H)
    pos, nrm = cast_planes(view, [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))], W, H)
    rng = np.random.default_rng(5)
    alb = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    alb[0, 0, :3] = 0  # the 0.01 floor of the demodulator
    pbr = np.zeros((H, W, 4), np.float32)
    assert (pos[..., 3] == 0).any() and (pos[..., 3] != 0).sum() > W * H // 3
    return view, pos, nrm, alb, pbr


def noise(seed, scale=1.0, shape=(H, W)):
    a = np.zeros(shape + (4,), np.float32)
    a[..., :3] = np.random.default_rng(seed).uniform(0.0, scale, shape + (3,)).astype(np.float32)
    return a


def with_samples(view, n):
    view.total_samples, view.accumulation_limit = n, 999999
    return view


def test_no_levels_no_flags_is_the_input_bit_for_bit(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    acc = noise(1, 3.0)
    r = dr.Denoiser()(acc, pos, nrm, alb, pbr, with_samples(view, 3), dr.default_params(flags=0, iterations=0))
    assert np.array_equal(bits(r["color"]), bits(r["input"]))
    assert np.array_equal(bits(r["input"][..., :3]), bits(acc[..., :3] / F(3.0)))
    assert np.array_equal(r["output"][..., :3][..., ::-1], dr.unorm8(dr.linear_to_srgb(r["color"][..., :3])))
    assert (r["output"][..., 3] == 0).all() and (r["color"][..., 3] == 0).all()


def test_one_level_on_a_plane_cuts_iid_noise_to_the_kernels_energy():
    """every weight is k: normals equal, plane distance 0, sigma_luminance 1e30. Sum of k^2 = (70/256)^2 = 0.0748"""
    n = 112
    y, x = np.mgrid[0:n, 0:n]
    pos = np.stack([x * 0.01, y * 0.01, np.full_like(x, -5.0, dtype=np.float64), np.ones_like(x)], axis=-1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1, 1], np.float32), (n, n, 1))
    view = with_samples(rr.ViewUniformData(), 1)
    view.view[:] = tuple(np.eye(4, dtype=np.float32).reshape(-1))
    acc = np.zeros((n, n, 4), np.float32)
    acc[..., :3] = np.random.default_rng(2).normal(1.0, 0.1, (n, n, 1)).astype(np.float32)
    r = dr.Denoiser()(acc, pos, nrm, np.zeros((n, n, 4), np.uint8), np.zeros((n, n, 4), np.float32), view,
                      dr.default_params(flags=0, iterations=1, sigma_luminance=1e30))
    inner = slice(8, 104)
    ratio = r["color"][inner, inner, 0].astype(np.float64).var() / acc[inner, inner, 0].astype(np.float64).var()
    print("variance ratio", ratio)
    assert abs(ratio / (70.0 / 256.0) ** 2 - 1.0) <= 0.2
    # and the filter's own estimate: var' = sum k^2 var / 1 with a constant var is the same factor of it
    v0, v1 = r["variance"][inner, inner].astype(np.float64), r["final_variance"][inner, inner].astype(np.float64)
    assert np.all(v1 <= v0.max() * (70.0 / 256.0) ** 2 * 1.0001)


@pytest.fixture(scope="module")
def crease():
    """an emissive floor and a black wall at a right angle, both large"""
    view = with_samples(plane_view((0.0, 1.2, 3.0), (0.0, 0.6, -2.0), W, H), 1)
    pos, nrm = cast_planes(view, [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0))], W, H)
    floor, wall = nrm[..., 1] == 1.0, nrm[..., 2] == 1.0
    assert floor.sum() > 100 and wall.sum() > 100 and (floor | wall).all()
    pbr = np.zeros((H, W, 4), np.float32)
    pbr[wall, 3] = 1.0
    acc = noise(3, 2.0)
    acc[wall] = 0.0
    return view, pos, nrm, pbr, acc, floor, wall


def test_no_weight_crosses_a_right_angle(crease):
    view, pos, nrm, pbr, acc, floor, wall = crease
    alb = np.full((H, W, 4), 255, np.uint8)
    r = dr.Denoiser()(acc, pos, nrm, alb, pbr, view, dr.default_params(flags=0))
    assert not bits(r["color"][wall]).any(), "no wall pixel has changed in any bit"
    assert not np.array_equal(bits(r["color"][floor]), bits(r["input"][floor])), "the floor was filtered"
    # a floor pixel is a filter of floor pixels only: whatever the wall's colours are, w_n = 0 multiplies them. (The wall's VARIANCE does
    # reach the 3 x 3 prefilter g of the floor pixels beside it, as the contract says; sigma_luminance = 1e30 takes g out of the weights.)
    p = dr.default_params(flags=0, sigma_luminance=1e30)
    a = dr.Denoiser()(acc, pos, nrm, alb, pbr, view, p)
    acc2 = acc.copy()
    acc2[wall, :3] = np.random.default_rng(9).uniform(0.0, 1e6, (int(wall.sum()), 3)).astype(np.float32)
    b = dr.Denoiser()(acc2, pos, nrm, alb, pbr, view, p)
    assert np.array_equal(bits(a["color"][floor]), bits(b["color"][floor]))
    assert np.isfinite(b["color"]).all()


def test_camera_at_rest_accumulates_the_running_mean(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 1)
    view.prev_frame_projection_view[:] = projection_view(view)
    p = dr.default_params(flags=dr.TEMPORAL, iterations=0, alpha_min=0.0)
    d, k = dr.Denoiser(), 8
    frames = [noise(20 + i, 4.0) for i in range(k)]
    for f in frames:
        r = d(f, pos, nrm, alb, pbr, view, p)
    geo = pos[..., 3] != 0
    assert np.array_equal(r["history"][geo], np.full(int(geo.sum()), F(k))) and not r["history"][~geo].any()
    assert r["kept"][geo].all()
    stack = np.stack([f[..., :3] for f in frames]).astype(np.float64)
    bound = 4 * k * 2.0 ** -23 * stack.max(axis=0)
    err = np.abs(r["temporal"][..., :3].astype(np.float64) - stack.mean(axis=0))
    assert (err[geo] <= bound[geo]).all(), (err[geo] / bound[geo]).max()
    assert np.array_equal(bits(r["temporal"][~geo]), bits(frames[-1][~geo]))


def test_history_off_the_image_and_after_a_reset_is_one(floor_frame):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 1)
    pv = np.array(projection_view(view), np.float32).reshape(4, 4)  # [column][row]
    geo = pos[..., 3] != 0
    p = dr.default_params(iterations=1)
    d = dr.Denoiser()
    view.prev_frame_projection_view[:] = tuple(pv.reshape(-1))
    d(noise(1), pos, nrm, alb, pbr, view, p)
    r = d(noise(2), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 2).all()
    off = pv.copy()
    off[:, 0] += F(10.0) * off[:, 3]  # clip x + 10 w: every point ten half-widths to the right
    view.prev_frame_projection_view[:] = tuple(off.reshape(-1))
    r = d(noise(3), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 1).all() and not r["kept"].any()
    view.prev_frame_projection_view[:] = tuple(pv.reshape(-1))
    assert (d(noise(4), pos, nrm, alb, pbr, view, p)["history"][geo] == 2).all()
    d.reset()
    r = d(noise(5), pos, nrm, alb, pbr, view, p)
    assert (r["history"][geo] == 1).all() and not r["kept"].any() and not r["history"][~geo].any()


@pytest.mark.parametrize("flags", [0, dr.TEMPORAL, dr.DEMODULATE, dr.TEMPORAL | dr.DEMODULATE])
def test_pixels_that_are_not_geometry_pass_through_bit_for_bit(floor_frame, flags):
    view, pos, nrm, alb, pbr = floor_frame
    view = with_samples(view, 2)
    view.prev_frame_projection_view[:] = projection_view(view)
    sky = pos[..., 3] == 0
    d = dr.Denoiser()
    for seed in (1, 2):
        acc = noise(seed, 5.0)
        r = d(acc, pos, nrm, alb, pbr, view, dr.default_params(flags=flags))
        want = bits(acc[..., :3] / F(2.0))[sky]
        for name in ("color", "input", "temporal"):
            assert np.array_equal(bits(r[name][..., :3])[sky], want), name
        assert not r["history"][sky].any() and not r["variance"][sky].any()
        assert not np.array_equal(bits(r["color"][~sky]), bits(r["input"][~sky]))

"""CPU: the numpy restatement of ray-traced ambient occlusion (tests/rtao_reference.py) held to properties and known answers on the oracle's
own G-buffer - the ray directions, a bare floor, the inside of a closed box, the radius, the filter. test_gpu_rtao.py holds the device to
the restatement and runs the known answers there."""
import numpy as np
import pytest

import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao
from hybrid_util import frame_view, synthetic_scene

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

W, H = ao.W, ao.H
F = np.float32


def world(scene):
    """the scene on the oracle, its view and the oracle's G-buffer of it"""
    cpu = oa.OracleRenderer(W, H)
    meshes = hr.upload_recorded(scene, cpu, scene.name != "hybrid_synthetic")
    view = frame_view(scene, W, H)
    return cpu, view, hr.gbuffer(cpu, meshes, view, W, H)


@pytest.fixture(scope="module")
def synthetic():
    return world(synthetic_scene())


def test_directions_are_unit_above_the_horizon_and_cosine_weighted(synthetic):
    _, view, g = synthetic
    rows, nn, d = ao.directions(g, view, 8)
    assert len(rows) > 1000 and np.isfinite(d).all()
    length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1))
    cos = (d.astype(np.float64) * nn.astype(np.float64)[:, None, :]).sum(axis=-1)
    print(f"{d.shape[0] * d.shape[1]} rays: max | |d| - 1 | = {np.abs(length - 1).max():.3e}, min dot(d, Nn) = {cos.min():.3e}, mean {cos.mean():.5f}")
    assert np.abs(length - 1).max() <= 2 * np.spacing(F(1.0))  # 2 ulp of 1
    assert (hr.dot(d, np.broadcast_to(nn[:, None, :], d.shape)) >= 0).all()  # in the float32 the kernel computes with
    assert abs(cos.mean() - 2.0 / 3.0) <= 0.01  # E[cos] of a cosine-weighted direction
    # the same view, the same directions: nothing but the view's frame number and the pixel enters them
    assert np.array_equal(ao.directions(g, view, 8)[2], d)
    assert np.array_equal(ao.directions(g, view, 3)[2], d[:, :3])


def test_a_bare_floor_is_unoccluded():
    cpu, view, g = world(ao.floor_scene())
    count, (pixels, rays, occluded), img = ao.image(cpu, g, view, ao.default_params(samples=8, radius=4.0))
    geo = g["position"][..., 3] != 0
    assert geo.any() and not geo.all() and pixels == geo.sum() and rays == 8 * pixels
    assert occluded == 0 and not count.any() and (img == 65535).all()


def test_inside_a_closed_box_every_ray_is_occluded():
    """the box of rtao_reference.inward_box_scene (half extents (1.0, 0.8, 1.2), diagonal 3.51 < the radius 4.0) from its camera at
    67 x 41 with 8 samples: no ray leaks through an edge"""
    cpu, view, g = world(ao.inward_box_scene())
    assert 2 * np.linalg.norm(ao.BOX_HALF) < ao.BOX_RADIUS
    geo = g["position"][..., 3] != 0
    assert geo.all() and (g["position"][..., 2] < -1.19).all(), "every primary ray meets the far wall"
    n = hr.normalize(g["normal"][..., :3].reshape(-1, 3))
    inward = np.array(ao.BOX_CENTRE, np.float32) - g["position"][..., :3].reshape(-1, 3)
    assert (hr.dot(n, inward) > 0).all(), "the normals point into the box"
    for strength in (1.0, 0.25):
        count, (pixels, rays, occluded), img = ao.image(cpu, g, view, ao.default_params(samples=8, radius=ao.BOX_RADIUS, strength=strength))
        assert pixels == W * H and occluded == rays == 8 * W * H and (count == 8).all()
        assert (img == int(np.rint(F(1.0 - strength) * F(65535.0)))).all()


def test_counts_grow_with_the_radius(synthetic):
    cpu, view, g = synthetic
    a, b, c = (ao.counts(cpu, g, view, 8, r)[0] for r in (0.25, 1.0, 4.0))
    print(f"occluded of {8 * (g['position'][..., 3] != 0).sum()} rays: {a.sum()} at 0.25, {b.sum()} at 1.0, {c.sum()} at 4.0")
    assert (a <= b).all() and (b <= c).all() and a.sum() < b.sum() < c.sum()
    assert c.min() == 0 and c.max() == 8, "unoccluded and fully occluded pixels both occur"


def test_the_filter(synthetic):
    _, _, g = synthetic
    _, cast = ao.normals(g)
    cast = cast.reshape(H, W)
    assert cast.any() and not cast.all()
    rng = np.random.default_rng(5)
    count = np.where(cast, rng.integers(0, 5, (H, W)), 0).astype(np.uint8)
    # radius 0 is the identity: unorm16 of the pixel's own ao, the sky 65535
    for strength in (1.0, 1.6):
        want = np.where(cast, np.rint(np.clip(1.0 - F(strength) * (count.astype(np.float32) / F(4.0)), 0.0, 1.0) * F(65535.0)), 65535)[::-1]
        assert np.array_equal(ao.resolve(g, count, 4, strength, 0), want.astype(np.uint16))
    # a constant count gives a constant image, the same at every radius; the sky stays 65535
    const = np.where(cast, 2, 0).astype(np.uint8)
    for r in (1, 2, 4):
        img = ao.resolve(g, const, 4, 1.0, r, 0.9, 0.05)[::-1]
        assert (img[cast] == 32768).all() and (img[~cast] == 65535).all(), r
    # thresholds nothing passes leave the centre tap alone: the identity again
    assert np.array_equal(ao.resolve(g, count, 4, 1.0, 4, 2.0, 0.05), ao.resolve(g, count, 4, 1.0, 0))
    # and the filter does something: with every tap let in, a pixel is the mean of its window
    wide = ao.resolve(g, count, 4, 1.0, 1, -1.0, np.inf)[::-1]
    y, x = np.argwhere(cast[2:-2, 2:-2] & cast[1:-3, 2:-2] & cast[2:-2, 1:-3] & cast[1:-3, 1:-3])[0] + 2
    taps = [F(1.0) - F(1.0) * (F(count[y + dy, x + dx]) / F(4.0)) for dy in (-1, 0) for dx in (-1, 0)]
    assert wide[y, x] == int(np.rint((((taps[0] + taps[1]) + taps[2]) + taps[3]) / F(4.0) * F(65535.0)))


def test_the_filter_on_frames_smaller_than_its_window():
    """a window of 8 x 8 taps over 5 x 3, 64 x 1 and 129 x 2 pixels: the taps outside the frame do not count"""
    for w, h in ((5, 3), (64, 1), (129, 2)):
        g = dict(position=np.ones((h, w, 4), np.float32), normal=np.tile(np.float32([0, 1, 0, 1]), (h, w, 1)))
        count = (np.arange(h * w).reshape(h, w) % 5).astype(np.uint8)
        img = ao.resolve(g, count, 4, 1.0, 4, 0.9, 0.05)[::-1]
        raw = F(1.0) - count.astype(np.float32) / F(4.0)
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
            total = F(0.0)
            taps = [(yy, xx) for yy in range(y - 4, y + 4) for xx in range(x - 4, x + 4) if 0 <= yy < h and 0 <= xx < w]
            for yy, xx in taps:
                total = total + raw[yy, xx]
            assert img[y, x] == int(np.rint(total / F(len(taps)) * F(65535.0))), (w, h, y, x)

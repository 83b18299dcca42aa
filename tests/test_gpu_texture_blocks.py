"""GPU: textures stored as overlapped blocks (csrc/texture_layout.h, option "texture_blocks" = 1, the default) against the same
textures stored as 8x8 tiles or rows (texture_blocks = 0). The layout changes where the four texels of a bilinear footprint lie, not
which four words enter the filter: accumulation, output image and the ray, hit and miss counts are equal BIT FOR BIT between two
contexts that differ in that option alone - through the wavefront of a batch (loop.frames: k_shade_hit), frame by frame (a lone
frame's later bounces in k_path_fused), with the fused kernel forced (fused_bounces = -1), and through one hybrid frame (the G-buffer
cast, the reflections' closest-hit shader and the deferred pass sample the same descriptors). The blocked context is also held to the
oracle at the tolerances of test_gpu_parity.py / test_gpu_hybrid.py.

Scenes, at 64 x 48, 2 frames of 5 bounces: the cornell scene of the parity suite, and a pair of facing walls of ten strips each, strip
k of either wall with texture k of the ten sizes tests/cpp/texture_layout_check.cpp walks on the host (1x1 .. 64x64 as w x h: smaller
than a block, a side of one block exactly, one texel more, neither side a multiple of anything), under uv that run from -3 to +3
across every strip: both mirror halves, negative coordinates, footprints at the texture's own edges where x0 == x1."""
import numpy as np
import pytest

import hybrid_reference as hr
import oracle_api as oa
import rust_renderer_amd as rr
import texture_f64 as tx
from hybrid_util import bits, frame_view, gbuf, read_all
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Mesh, Model, Scene, quad
from util import L2_TOL, per_pixel_l2

pytestmark = pytest.mark.gpu
W, H = 64, 48
FRAMES, BOUNCES = 2, 5
SIZES = [(1, 1), (2, 2), (3, 5), (7, 3), (8, 4), (9, 5), (15, 22), (16, 8), (8, 24), (64, 64)]  # w x h
GAP, STRIP, HALF_HEIGHT = 3.0, 0.4, 1.5
F = np.float32


def walls_scene():
    textures = [tx.random_texture(h, w, seed=0xB10C + k) for k, (w, h) in enumerate(SIZES)]
    meshes = []
    for wall in range(2):
        for k in range(len(SIZES)):
            x0 = (k - len(SIZES) / 2) * STRIP
            if wall == 0:  # faces +z
                v, i = quad((x0, -HALF_HEIGHT, 0.0), (STRIP, 0.0, 0.0), (0.0, 2 * HALF_HEIGHT, 0.0), nu=2, nv=3)
            else:  # faces -z
                v, i = quad((x0 + STRIP, -HALF_HEIGHT, GAP), (-STRIP, 0.0, 0.0), (0.0, 2 * HALF_HEIGHT, 0.0), nu=2, nv=3)
            v["uv"] = v["uv"] * F(6.0) - F(3.0)
            kind = rr.LAMBERTIAN if (k + wall) % 3 else rr.METAL  # metal strips: the hybrid frame's reflection rays sample too
            meshes.append(Mesh(v, i, kind, 0.1, (0.95, 0.9, 0.85, 1.0), k, name=f"wall{wall}_strip{k}"))
    cam = Camera((0.0, 0.0, 0.15), (0.0, 0.0, GAP), 60.0, W / H, 0.01, 1000.0)
    return Scene("texture_block_walls", [(Model(meshes, textures), None)], [(0.3, 0.4, 1.5), (-1.0, -0.5, 2.0)], cam, dict(sky_enabled=1))


SCENES = {"walls": walls_scene, "cornell": lambda: rr.scenes.cornell_scene(subdivisions=2, tex_size=16)}
_CACHE = {}


def scene_named(name):
    if name not in _CACHE:
        _CACHE[name] = SCENES[name]()
    return _CACHE[name]


def device(scene, blocks, options=()):
    gpu = rr.Renderer(W, H)
    gpu.set_option("texture_blocks", blocks)  # read when a texture is added: before the upload
    for k, v in options:
        gpu.set_option(k, v)
    hr.upload_recorded(scene, gpu, True)  # Renderer.initialize's 1x1 default maps first: every material carries all four maps
    return gpu


def mask_of(scene):
    return rr.PASS_ALL if scene.lights else rr.PASS_REFERENCE_PT


def path_trace(renderer, scene, mode):
    loop = rr.FrameLoop(renderer, scene.make_view(W, H, num_bounces=BOUNCES, samples_per_frame=1))
    if mode == "batched":
        loop.frames(FRAMES, mask_of(scene))
    else:
        for _ in range(FRAMES):  # one frame per call, the GPU idle before each
            loop.frame(mask_of(scene))
            renderer.synchronize()
    s = renderer.get_stats()
    return dict(accumulation=renderer.read_accumulation(), output=renderer.read_output_bgra8(), rays=list(s.rays), hits=s.closest_hits, misses=s.misses)


def oracle_frames(name):
    """the oracle's frames of a scene, rendered once and shared by the modes (batched frames equal frame-by-frame ones bit for bit)"""
    if ("oracle", name) not in _CACHE:
        scene = scene_named(name)
        cpu = oa.OracleRenderer(W, H)
        hr.upload_recorded(scene, cpu, True)
        got = path_trace(cpu, scene, "frame_by_frame")
        got["accumulation"].setflags(write=False)
        _CACHE[("oracle", name)] = got
    return _CACHE[("oracle", name)]


MODES = {"batched": (), "frame_by_frame": (), "fused_always": (("fused_bounces", -1),)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SCENES))
def test_path_traced_frames_are_the_same_bit_for_bit(name, mode):
    scene = scene_named(name)
    rows = path_trace(device(scene, 0, MODES[mode]), scene, mode)
    blocked = path_trace(device(scene, 1, MODES[mode]), scene, mode)
    assert np.array_equal(bits(blocked["accumulation"]), bits(rows["accumulation"])), f"{(blocked['accumulation'] != rows['accumulation']).any(-1).sum()} pixels differ"
    assert np.array_equal(blocked["output"], rows["output"])
    assert blocked["rays"] == rows["rays"] and blocked["hits"] == rows["hits"] and blocked["misses"] == rows["misses"]
    assert blocked["hits"] > FRAMES * W * H, "more hits than primary rays: textures are sampled at later bounces too"
    # and the oracle's, at the parity suite's tolerance
    cpu = oracle_frames(name)
    assert np.isfinite(blocked["accumulation"]).all()
    l2 = per_pixel_l2(blocked["accumulation"] / FRAMES, cpu["accumulation"] / FRAMES)
    print(f"{name} [{mode}]: per-pixel L2 against the oracle {l2:.3e}")
    assert l2 <= L2_TOL, f"per-pixel L2 {l2}"
    assert blocked["rays"] == cpu["rays"] and blocked["hits"] == cpu["hits"] and blocked["misses"] == cpu["misses"]
    assert np.abs(blocked["output"].astype(np.int32) - cpu["output"].astype(np.int32)).max() <= 1


@pytest.mark.parametrize("name", list(SCENES))
def test_a_hybrid_frame_is_the_same_bit_for_bit(name):
    scene = scene_named(name)
    view = frame_view(scene, W, H)
    images = []
    for blocks in (0, 1):
        gpu = device(scene, blocks)
        gpu.render_hybrid(view, rr.HYBRID_FRAME)
        images.append((read_all(gpu), gbuf(gpu)))
    (rows, _), (blocked, g) = images
    for k in rows:
        assert np.array_equal(np.ascontiguousarray(rows[k]).view(np.uint8), np.ascontiguousarray(blocked[k]).view(np.uint8)), f"hybrid image {k}"
    # the cast G-buffer against the oracle, as test_gpu_hybrid.py compares it: bit for bit, the albedo target byte for byte
    cpu = oa.OracleRenderer(W, H)
    meshes = hr.upload_recorded(scene, cpu, True)
    ref = hr.gbuffer(cpu, meshes, view, W, H)
    for k in ("position", "normal", "pbr"):
        assert np.array_equal(bits(g[k]), bits(ref[k])), k
    assert np.array_equal(g["albedo"], ref["albedo"])
    hit = g["position"][..., 3] == 1.0
    assert hit.mean() > 0.5 and len(np.unique(g["albedo"][hit].reshape(-1, 4), axis=0)) > 50, "the albedo target carries the maps' texels"


def test_every_strip_of_both_walls_is_reached():
    """what the comparisons on the walls rest on: rays from the camera reach every strip of the far wall, rays back from it every strip
    of the near one, and the strips' uv span -3 .. +3"""
    scene = scene_named("walls")
    gpu = device(scene, 1)
    xs = (np.arange(len(SIZES)) - len(SIZES) / 2 + 0.3) * STRIP  # (off the strips' middle, where two of their triangles share an edge)
    rays = np.zeros((2 * len(xs), 8), F)
    rays[:, 3], rays[:, 7] = 0.001, 10000.0
    rays[: len(xs), 0:3], rays[len(xs):, 0:3] = (0.0, 0.0, 0.15), (0.0, 0.0, GAP - 0.15)
    rays[: len(xs), 4], rays[: len(xs), 5], rays[: len(xs), 6] = xs, 0.2, GAP - 0.15
    rays[len(xs):, 4], rays[len(xs):, 5], rays[len(xs):, 6] = xs, -0.2, -(GAP - 0.15)
    _, mesh, _ = gpu.trace_closest(rays)
    assert list(mesh) == [len(SIZES) + k for k in range(len(SIZES))] + list(range(len(SIZES)))
    for m in scene.models[0][0].meshes:
        assert m.vertices["uv"][:, :2].min() == -3.0 and m.vertices["uv"][:, :2].max() == 3.0
    assert [t.shape[:2] for t in scene.models[0][0].textures] == [(h, w) for w, h in SIZES]


def test_texture_blocks_is_read_when_a_texture_is_added():
    """the option lays out the textures added after it: a context may hold both kinds, and renders as either alone does"""
    scene = scene_named("walls")
    want = path_trace(device(scene, 1), scene, "batched")
    mixed = rr.Renderer(W, H)
    model = scene.models[0][0]
    mixed.initialize()
    add = mixed.add_texture

    def alternating(texture):
        mixed.set_option("texture_blocks", alternating.count % 2)
        alternating.count += 1
        return add(texture)

    alternating.count = 0
    mixed.add_texture = alternating
    try:
        scene.upload(mixed)
    finally:
        del mixed.add_texture
    assert alternating.count == len(model.textures)
    got = path_trace(mixed, scene, "batched")
    assert np.array_equal(bits(got["accumulation"]), bits(want["accumulation"])) and got["rays"] == want["rays"]

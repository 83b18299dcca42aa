"""GPU: texture sampling on the device (csrc/device_math.h sample_texture_pre, the uploader uh_add_texture_rgba8) at the storage
layouts, descriptor counts and uv that no scene of the suite reaches: textures stored as rows (a side that is no multiple of 8), tiled
textures that are not square, more descriptors than the shading kernels stage in LDS (64 textures; 192 / 128 meshes), and uv that are
negative, far past 1, on texel centres and edges, and past the sampler's 1e9 guard. Bit for bit against the oracle, and - independent of
every float32 reading - inside the envelope of the float64 sampler of tests/texture_f64.py.

How the filter is read out of the path tracer. A path that ends on a DiffuseLight does NOT carry its texel: reference.rchit:85-89 (and
path_shading.h material_scatter, oracle.cpp closest_hit_shader) set its colour to 1. What carries it: a Lambertian quad with base
colour 1 under a sun that nothing shadows, sky and lights off, two bounces. Bounce 0 multiplies the throughput (1) by the filtered
texel and its sun ray adds that throughput to the radiance (0): rgen:48, :69-76. Bounce 1 leaves the quad, misses, and adds
throughput * 0 (rmiss with the sky off). The accumulation of the first frame is 0 + texel + 0: the filtered texel, exactly.

Where the path hit. The G-buffer pass casts through pixel centres while the path tracer jitters its primary rays (rgen:31), so
read_gbuffer_position() is not the path's hit point. The test rebuilds each pixel's jittered primary ray from the oracle's unit entry
points (initRNG, randomFloat, the primary ray), asks the DEVICE for its hit distance (trace_closest) and takes origin + t * direction
in float32, as k_shade_hit does (rgen:59)."""
import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
import texture_f64 as tx
import forward_reference as fw
import hybrid_reference as hr
import test_gpu_forward
import test_gpu_gbuffer_raster
from hybrid_util import SyntheticScene, assert_reflections, bits, frame_view, gbuf, hybrid_view
from rust_renderer_amd.camera import Camera
from rust_renderer_amd.scenes import Mesh, Model, Scene, icosphere, merge, quad

pytestmark = pytest.mark.gpu
W, H = 67, 41
PT = rr.PASS_REFERENCE_PT
OPTION_SETS = {"default": {}, "wavefront": {"fused_bounces": 0}}  # a lone frame's later bounces in k_path_fused / every bounce in k_shade_hit
SHAPE_IDS = [f"{h}x{w}" for h, w in tx.SHAPES]
F = np.float32

# ---- the quad of parts a and b ------------------------------------------------------------------------------------------------
# It stands away from the origin on purpose. The device interpolates uv from the hit's barycentrics: an error of a few 2^-24 of
# the uv span (6.8), wherever the quad stands. The bound of part a is one float32 spacing of the hit POSITION, which vanishes towards
# the coordinate planes; at x, y in [32, 64) it is 3.8e-6 everywhere - in uv (1.36 and 2.2 per unit) 5e-6 to 8e-6: half of it is the
# position's own rounding, the rest holds the interpolation's few 1e-6.
X0, X1, Y0, Y1 = 37.0, 42.0, 38.0, 41.0
U0, U1, V0, V1 = (float(F(a)) for a in (-2.9, 3.9, -2.8, 3.8))  # at the quad's corners; the frame sees about [-2.5, 3.5] of both
CAMERA = ((X0 + X1) / 2, (Y0 + Y1) / 2, 2.338)                  # 60 degrees at this distance: 2.7 of the quad's 3 units of height
READ_OUT = dict(sky_enabled=0, lights_enabled=0, sun_shadow_enabled=1, num_bounces=2, samples_per_frame=1)


def _camera():
    return Camera(CAMERA, (CAMERA[0], CAMERA[1], 0.0), 60.0, W / H, 0.01, 1000.0)


def _view(scene):
    v = scene.make_view(W, H, **READ_OUT)
    v.sun_dir[:] = (0.0, 0.0, 1.0)  # along the quad's normal: no sun ray is shadowed
    return v


def filter_scene(tex):
    """one Lambertian quad facing the camera and filling the frame, its vertex uv assigned directly"""
    v, i = quad((X0, Y0, 0.0), (X1 - X0, 0.0, 0.0), (0.0, Y1 - Y0, 0.0))
    s, t = (v["pos"][:, 0] - F(X0)) / F(X1 - X0), (v["pos"][:, 1] - F(Y0)) / F(Y1 - Y0)  # 0 or 1
    v["uv"][:, 0], v["uv"][:, 1] = np.where(s == 0, F(U0), F(U1)), np.where(t == 0, F(V0), F(V1))
    return Scene("texture_filter", [(Model([Mesh(v, i, rr.LAMBERTIAN, 0.0, (1.0, 1.0, 1.0, 1.0), 0)], [tex]), None)], [], _camera())


CELLS_X, CELLS_Y = 8, 5


def cell_uv(h, w):
    """the 40 constant (u, v) of part b's cells, float32: four past the 1e9 guard in one axis or both, then half-texel steps k * 0.5 / w,
    k * 0.5 / h - texel edges (k even) and centres (k odd) - at the texture's own edges, in the mirrored half, negative and past 1"""
    rng = np.random.default_rng([7, h, w])
    ku = [0, 1, -1, 2 * w, 2 * w - 1, 2 * w + 1, -2 * w, 4 * w, -1 - 2 * w, w] + list(rng.integers(-5 * w, 7 * w + 1, 26))
    kv = [0, 1, -1, 2 * h - 1, 2 * h, -2 * h, 2 * h + 1, -1 - 2 * h, 4 * h, h] + list(rng.integers(-5 * h, 7 * h + 1, 26))
    uv = [(1e12, 1e12), (-1e12, 0.3), (0.3, 1e12), (1e12, -1e12)] + [(a * 0.5 / w, b * 0.5 / h) for a, b in zip(ku, kv)]
    return np.array(uv, np.float64).astype(F), np.array([(0, 0)] * 4 + list(zip(ku, kv)))


def cells_scene(tex):
    """the same quad cut into 8 x 5 cells, every vertex of a cell carrying that cell's uv: whatever the barycentrics, the interpolated
    uv is the cell's constant but for the rounding of (c * b0 + c * b1) + c * b2"""
    uv, _ = cell_uv(*tex.shape[:2])
    parts = []
    for k in range(CELLS_X * CELLS_Y):
        cx, cy = k % CELLS_X, k // CELLS_X
        dx, dy = (X1 - X0) / CELLS_X, (Y1 - Y0) / CELLS_Y
        v, i = quad((X0 + cx * dx, Y0 + cy * dy, 0.0), (dx, 0.0, 0.0), (0.0, dy, 0.0))
        v["uv"][:] = uv[k]
        parts.append((v, i))
    v, i = merge(parts)  # two triangles per cell, in cell order: cell = prim // 2
    return Scene("texture_cells", [(Model([Mesh(v, i, rr.LAMBERTIAN, 0.0, (1.0, 1.0, 1.0, 1.0), 0)], [tex]), None)], [], _camera())


_RAYS = {}


def path_primary_rays(view):
    """the jittered primary rays of the frame `view` describes (its total_samples as rendered), one per pixel, from the oracle's unit
    entry points: rgen:24-38. Returns (rays (H * W, 8), seeds (H * W,): the RNG word the closest-hit shader starts from, rgen:30)"""
    key = bytes(view)
    if key not in _RAYS:
        frame = oa.frame_number(view)
        rays, seeds = np.zeros((H * W, 8), F), np.zeros(H * W, np.uint32)
        for py in range(H):
            for px in range(W):
                s = oa.init_rng(px, py, W, frame)
                (jx, jy), _ = oa.random_floats(s, 2)
                r = oa.primary_ray(view, W, H, px, py, float(jx), float(jy))
                rays[py * W + px, 0:3], rays[py * W + px, 4:7], seeds[py * W + px] = r[:3], r[3:], s
        rays[:, 3], rays[:, 7] = 0.001, 10000.0
        _RAYS[key] = (rays, seeds)
    return _RAYS[key]


def first_frame(renderer, scene):
    loop = rr.FrameLoop(renderer, _view(scene))
    loop.frame(PT)
    return renderer.read_accumulation(), loop.view


_ORACLE = {}


def oracle_frame(kind, shape, scene):
    """the oracle's first frame of a shape's scene, rendered once and shared by the option sets"""
    if (kind, shape) not in _ORACLE:
        cpu = scene.upload(oa.OracleRenderer(W, H))
        acc, _ = first_frame(cpu, scene)
        assert cpu.get_stats().misses == W * H, "every path's second ray leaves the quad; no primary ray misses it"
        acc.setflags(write=False)
        _ORACLE[(kind, shape)] = acc
    return _ORACLE[(kind, shape)]


def device_frame(scene, options):
    gpu = rr.Renderer(W, H)
    for k, v in options.items():
        gpu.set_option(k, v)
    scene.upload(gpu)
    acc, view = first_frame(gpu, scene)
    rays, _ = path_primary_rays(view)
    tuv, mesh, prim = gpu.trace_closest(rays)
    assert (mesh == 0).all(), "the quad fills the frame"
    hit = rays[:, 0:3] + tuv[:, 0:1] * rays[:, 4:7]  # float32, as rgen:59
    return acc.reshape(-1, 4), hit, prim


# ---- a. the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", list(OPTION_SETS), ids=list(OPTION_SETS))
@pytest.mark.parametrize("shape", tx.SHAPES, ids=SHAPE_IDS)
def test_filter_equals_the_oracle_and_lies_in_the_float64_envelope(shape, options):
    """Worst use of the widened envelope on an MI355X (0 = its middle, 1 = its edge), both option sets alike since the frames are
    bit-identical: see DESIGN.md "Texture sampling on the device"."""
    h, w = shape
    tex = tx.random_texture(h, w)
    scene = filter_scene(tex)
    acc, hit, _ = device_frame(scene, OPTION_SETS[options])
    # 1. bit for bit the oracle's
    want = oracle_frame("filter", shape, scene).reshape(-1, 4)
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), f"{(acc != want).any(-1).sum()} pixels differ from the oracle"
    # 2. inside the float64 envelope at the uv of the hit point (the quad's affine map), the box one float32 spacing of the position wide
    p = hit.astype(np.float64)
    su, sv = (U1 - U0) / (X1 - X0), (V1 - V0) / (Y1 - Y0)
    u, v = U0 + (p[:, 0] - X0) * su, V0 + (p[:, 1] - Y0) * sv
    du, dv = np.spacing(hit[:, 0]).astype(np.float64) * su, np.spacing(hit[:, 1]).astype(np.float64) * sv
    lo, hi = tx.envelope(tex, u, v, du, dv)
    got = acc[:, :3].astype(np.float64)
    use = tx.envelope_use(got, lo, hi, tx.WIDEN)
    excess = np.maximum(lo - got, got - hi).max() / tx.ULP1
    print(f"texture {h}x{w} [{options}]: worst use of the widened envelope {use.max():.3f}; worst excess over the unwidened one {excess:.2f} ulp")
    assert (got >= lo - tx.WIDEN).all() and (got <= hi + tx.WIDEN).all(), f"outside the float64 envelope: use {use.max():.3f}"
    assert np.abs(hit[:, 2]).max() < 1e-5, "the hit points lie on the quad's plane"
    # 3. what the frame reached, by the float64 reading's own addresses
    i, j = tx.footprint(tex, u, v)
    for name, k, n in (("u", i, w), ("v", j, h)):
        half = np.mod(k, 2 * n) >= n
        assert half.any() and (~half).any(), f"both mirror halves in {name}"
    assert (u < 0).any() and (v < 0).any() and (u > 1).any() and (v > 1).any(), "negative uv and uv past 1"
    x0, y0 = tx.mirrored_repeat(i, w), tx.mirrored_repeat(j, h)
    assert len(np.unique(y0 * w + x0)) >= min(h * w, 200), "the frame's footprints start at most of the texture's texels"
    if w % 8 == 0 and h % 8 == 0:  # tiled: texels beyond the first tile in each axis that has more than one - in both at once where it can be
        assert w == 8 or (x0 >= 8).any()
        assert h == 8 or (y0 >= 8).any()
        assert w == 8 or h == 8 or ((x0 >= 8) & (y0 >= 8)).any()


# ---- b. extreme uv ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", list(OPTION_SETS), ids=list(OPTION_SETS))
@pytest.mark.parametrize("shape", tx.SHAPES, ids=SHAPE_IDS)
def test_texel_centres_edges_and_uv_past_the_guard(shape, options):
    """|u * w - 0.5| >= 1e9 returns black (device_math.h, oracle.cpp; the reference's GLSL leaves such coordinates to the sampler) - finite
    uv of 1e12 in one axis or both; exact half-texel uv give the texel itself (centres) or a mean of texels (edges)"""
    h, w = shape
    tex = tx.random_texture(h, w)
    scene = cells_scene(tex)
    acc, _, prim = device_frame(scene, OPTION_SETS[options])
    want = oracle_frame("cells", shape, scene).reshape(-1, 4)
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), f"{(acc != want).any(-1).sum()} pixels differ from the oracle"
    uv, steps = cell_uv(h, w)
    cell = (prim // 2).astype(np.int64)
    assert set(np.unique(cell)) == set(range(CELLS_X * CELLS_Y)), "every cell is seen"
    past = cell < 4
    assert not acc[past].any() and not want[past].any(), "past the guard: black on the device and on the oracle"
    # the rest: inside the float64 envelope at the cell's uv. The interpolation of a constant c: b0 + b1 + b2 is 1 within 2^-23 (two
    # roundings of 1 - u - v), three products and two sums round to 2^-24 of |c| each: within 7 * 2^-24 |c| <= 7 spacing(c); 8 is asked
    c = uv[cell[~past]].astype(np.float64)
    spread = 8.0 * np.spacing(np.abs(uv[cell[~past]])).astype(np.float64)
    lo, hi = tx.envelope(tex, c[:, 0], c[:, 1], spread[:, 0], spread[:, 1])
    got = acc[~past, :3].astype(np.float64)
    print(f"texture {h}x{w} [{options}]: worst use of the widened envelope at half-texel uv {tx.envelope_use(got, lo, hi, tx.WIDEN).max():.3f}")
    assert (got >= lo - tx.WIDEN).all() and (got <= hi + tx.WIDEN).all()
    # the float64 reading at the exact texel centres is the texel itself, and the device is next to it
    t = tex[..., :3].astype(np.float64) / 255.0
    centres = [k for k in range(4, CELLS_X * CELLS_Y) if steps[k][0] % 2 and steps[k][1] % 2]
    assert len(centres) >= 3
    for k in centres:
        a, b = int(steps[k][0]), int(steps[k][1])
        texel = t[tx.mirrored_repeat((b - 1) // 2, h), tx.mirrored_repeat((a - 1) // 2, w)]
        assert np.abs(tx.sample(tex, [a * 0.5 / w], [b * 0.5 / h])[0] - texel).max() < 1e-12
        # per axis, in spacings of c: half for c's own rounding to float32, 7 for the interpolation, 2 for the sampler's coordinate
        # (texture_f64.WIDEN) - under 10; in texels that is times the size, and a texel away the value differs by at most 1
        su, sv = (float(s) for s in np.spacing(np.abs(uv[k])))
        near = 10.0 * (su * w + sv * h) + tx.WIDEN
        assert np.abs(acc[cell == k, :3].astype(np.float64) - texel).max() <= near


# ---- c. more descriptors than the shading kernels keep in LDS -------------------------------------------------------------------
GAP = 4.0
N_MESHES, N_TEXTURES = 200, 70


def walls_scene():
    """two facing walls of 10 x 10 Lambertian quads each, 200 meshes, mesh k with texture k % 70 of 70 textures that cycle through the
    shapes. The cells of the outermost ring reach out to +-1000, so that no path of these frames leaves between the walls: the sky is
    on as the frame's flags have it, but its integral - the one term that is not bit-exact between the device's and the host's math
    libraries - is never evaluated (asserted: no miss). The meshes the LDS tables do not hold (index >= 192 in k_shade_hit, >= 128 in
    k_path_fused; textures >= 64: meshes 64..69 and 134..139) take the cells nearest to the walls' centres, alternating between the
    walls, so that primary rays and bounce rays both find them."""
    textures = [tx.random_texture(*tx.SHAPES[k % len(tx.SHAPES)], seed=0xC00 + k) for k in range(N_TEXTURES)]
    edges = np.array([-1000.0, -4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 1000.0])
    cells = sorted(((r, c) for r in range(10) for c in range(10)), key=lambda rc: (max(abs(rc[0] - 4.5), abs(rc[1] - 4.5)), rc))
    first = list(range(192, 200)) + list(range(134, 140)) + list(range(64, 70))
    order = first + [k for k in range(N_MESHES - 1, -1, -1) if k not in first]
    slot = {k: s for s, k in enumerate(order)}
    meshes = []
    for k in range(N_MESHES):
        wall, (r, c) = slot[k] % 2, cells[slot[k] // 2]
        x0, x1, y0, y1 = edges[c], edges[c + 1], edges[r], edges[r + 1]
        if wall == 0:
            v, i = quad((x0, y0, 0.0), (x1 - x0, 0.0, 0.0), (0.0, y1 - y0, 0.0))
        else:
            v, i = quad((x1, y0, GAP), (x0 - x1, 0.0, 0.0), (0.0, y1 - y0, 0.0))
        v["uv"] = v["uv"] * F(4.0) - F(1.5)  # [-1.5, 2.5]: negative, past 1, both mirror halves
        tint = (0.9, 0.8 + 0.001 * (k % 7), 0.7 + 0.002 * (k % 5), 1.0)
        meshes.append(Mesh(v, i, rr.LAMBERTIAN, 0.0, tint, k % N_TEXTURES, name=f"wall{wall}_{r}_{c}"))
    lights = [(0.5, 0.3, 2.0), (-1.5, 1.0, 1.0), (2.0, -1.0, 3.0)]
    cam = Camera((0.0, 0.0, 0.2), (0.0, 0.0, GAP), 60.0, W / H, 0.01, 1000.0)
    flags = dict(sky_enabled=1, sun_shadow_enabled=0, lights_enabled=1, use_ris_light_sampling=1, num_bounces=3, samples_per_frame=1)
    return Scene("texture_walls", [(Model(meshes, textures), None)], lights, cam, flags)


def _state(r):
    return [r.read_accumulation().view(np.uint32)] + [r.read_reservoirs(k).view(np.uint8) for k in range(3)]


@pytest.fixture(scope="module")
def walls():
    """the scene, the oracle's state after 2 and after 4 frames, and the oracle itself (for its ray queries)"""
    scene = walls_scene()
    cpu = scene.upload(oa.OracleRenderer(W, H))
    loop = rr.FrameLoop(cpu, scene.make_view(W, H))
    states, counts = {}, {}
    for frames in (2, 4):
        for _ in range(2):
            loop.frame(rr.PASS_ALL)
        states[frames] = _state(cpu)
        counts[frames] = list(cpu.get_stats().rays)
    assert cpu.get_stats().misses == 0, "no path leaves between the walls: the sky integral is never evaluated"
    return scene, states, cpu, counts


def _same(gpu, want):
    for k, (a, b) in enumerate(zip(_state(gpu), want)):
        assert np.array_equal(a, b), ("accumulation", "reservoirs 0", "reservoirs 1", "reservoirs 2")[k]


@pytest.mark.parametrize("mode", ["default", "wavefront", "fused_always", "batch_of_4"])
def test_descriptors_beyond_the_lds_tables(walls, mode):
    scene, states, cpu, counts = walls
    gpu = rr.Renderer(W, H)
    for k, v in {"default": {}, "wavefront": {"fused_bounces": 0}, "fused_always": {"fused_bounces": -1}, "batch_of_4": {"batch_frames": 4}}[mode].items():
        gpu.set_option(k, v)
    scene.upload(gpu)
    assert gpu.get_stats().bvh_triangles == 2 * N_MESHES
    loop = rr.FrameLoop(gpu, scene.make_view(W, H))
    if mode == "batch_of_4":
        loop.frames(4, rr.PASS_ALL)
        done = 4
    else:
        for _ in range(2):  # one frame per call, the GPU idle before each: the default takes its later bounces through k_path_fused
            loop.frame(rr.PASS_ALL)
            gpu.synchronize()
        done = 2
    _same(gpu, states[done])
    assert list(gpu.get_stats().rays) == counts[done] and gpu.get_stats().misses == 0


def test_the_walls_frames_reach_the_descriptors_beyond_the_lds_tables(walls):
    """the coverage the comparison above rests on, from the device's own hits on the first frame's primary rays and from the oracle's
    closest-hit shader and ray query for the rays of bounce 1"""
    scene, states, cpu, _ = walls
    gpu = scene.upload(rr.Renderer(W, H))
    view = scene.make_view(W, H)
    view.total_samples = 1  # the first frame
    rays, seeds = path_primary_rays(view)
    tuv, mesh, prim = gpu.trace_closest(rays)
    tc, mc, pc = cpu.trace_closest(rays)
    assert np.array_equal(mesh, mc) and np.array_equal(prim, pc) and np.array_equal(tuv.view(np.uint32), tc.view(np.uint32))
    assert (mesh != 0xFFFFFFFF).all()
    hit0 = set(int(m) for m in np.unique(mesh))
    assert any(m >= 192 for m in hit0), "bounce 0 (k_shade_hit): a mesh record beyond its 192 in LDS"
    assert any(m % N_TEXTURES >= 64 for m in hit0), "bounce 0: a texture descriptor beyond the 64 in LDS"
    # bounce 1: rgen:59-61 on the payload of the closest-hit shader
    nxt = np.zeros_like(rays)
    for k in range(len(rays)):
        out, _ = cpu.closest_hit_shader(int(mesh[k]), int(prim[k]), float(tuv[k, 0]), float(tuv[k, 1]), float(tuv[k, 2]), rays[k, 4:7], int(seeds[k]))
        assert out[7] == 1.0, "a Lambertian wall scatters every path that meets it from the front"
        origin = rays[k, 0:3] + tuv[k, 0] * rays[k, 4:7]
        nxt[k, 0:3], nxt[k, 4:7] = oa.offset_ray(origin, out[8:11]), out[4:7]
    nxt[:, 3], nxt[:, 7] = 0.001, 10000.0
    _, m1, _ = cpu.trace_closest(nxt)
    assert (m1 != 0xFFFFFFFF).all(), "as the frames' miss count says: every ray of bounce 1 meets the other wall"
    hit1 = set(int(m) for m in np.unique(m1))
    assert any(m >= 192 for m in hit1) and any(128 <= m < 192 for m in hit1), "bounce 1 (k_path_fused): mesh records beyond its 128 in LDS"
    assert any(m % N_TEXTURES >= 64 and m >= 128 for m in hit1), "bounce 1: a texture descriptor beyond the 64 in LDS, on such a mesh"


# ---- d. the raster and hybrid consumers (forward.hip, hybrid_kernels.hip, hybrid_shading.h) -------------------------------------
def _normal_map(h, w):
    """hybrid_util._normal_map at any size: a bumpy tangent-space normal map, z dominant"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    nx, ny = 0.45 * np.sin(x * 0.7), 0.45 * np.cos(y * 0.5)
    nz = np.sqrt(np.maximum(1.0 - nx * nx - ny * ny, 0.0))
    rgba = np.stack([(nx * 0.5 + 0.5) * 255, (ny * 0.5 + 0.5) * 255, (nz * 0.5 + 0.5) * 255, np.full_like(nx, 255)], axis=-1)
    return np.ascontiguousarray(np.rint(rgba).astype(np.uint8))


class OddMapsScene(SyntheticScene):
    """hybrid_util.SyntheticScene - its meshes, instances and materials - with other maps only: diffuse 9 x 17 (rows), normal 12 x 20
    (rows), metallic-roughness 8 x 24 (tiled, not square), occlusion 1 x 1, and the floor - the mesh that fills most of the frame; the
    box-side quad stands edge-on to this camera - with a 16 x 8 (tiled) diffuse map under a uv scale that reaches uv of -3"""

    def upload(self, renderer):
        renderer.default_diffuse_map()
        diffuse, diffuse_floor = renderer.add_texture(tx.random_texture(9, 17, seed=21)), renderer.add_texture(tx.random_texture(16, 8, seed=22))
        nmap = renderer.add_texture(_normal_map(12, 20))
        mr_map = tx.random_texture(8, 24, seed=23)
        mr_map[..., :3] = 48 + mr_map[..., :3] // 2  # metallic and roughness away from 0: the deferred terms stay finite
        mr, occlusion = renderer.add_texture(mr_map), renderer.add_texture(np.array([[[200, 190, 180, 255]]], np.uint8))

        def mat(kind, diffuse_map, base=(1.0, 1.0, 1.0, 1.0)):
            m = rr.make_material(kind, 0.0, base, diffuse_map=diffuse_map)
            m.normal_map, m.metallic_roughness_map, m.occlusion_map = nmap, mr, occlusion
            return m

        fv, fi = quad((-6.0, 0.0, 6.0), (12.0, 0.0, 0.0), (0.0, 0.0, -12.0), nu=6, nv=6, uv_scale=(-3.0, 3.0))
        fv["tangent"][:, :3] = (1.0, 0.0, 0.0)
        renderer.add_mesh(fv, fi, mat(rr.METAL, diffuse_floor, (0.9, 0.8, 0.7, 1.0)))
        sv, si = icosphere(2)
        rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], np.float32)
        renderer.add_mesh(sv, si, mat(rr.LAMBERTIAN, diffuse, (0.5, 0.9, 0.4, 1.0)), rr.transform3x4((1.4, 0.6, 0.9), (-1.5, 0.8, 0.0), rot))
        qv, qi = quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), nu=3, nv=3, uv_scale=(2.0, 2.0))
        qv["tangent"][:, :3] = (1.0, 0.0, 0.0)
        rot2 = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]], np.float32) @ np.array([[0.96, 0.0, -0.28], [0.0, 1.0, 0.0], [0.28, 0.0, 0.96]], np.float32)
        renderer.add_mesh(qv, qi, mat(rr.LAMBERTIAN, diffuse), rr.transform3x4((1.0, 0.7, 1.6), (2.2, 1.0, -1.0), rot2))
        renderer.add_mesh(sv, si, mat(rr.METAL, diffuse), rr.transform3x4((0.7, 0.7, 0.7), (0.6, 0.7, 1.4)))
        renderer.initialize_raytracing()
        return renderer


def odd_maps_scene():
    cam = Camera((0.0, 2.2, 6.5), (0.0, 0.9, 0.0), 60.0, W / H, 0.01, 1000.0)  # hybrid_util.synthetic_scene's camera
    return OddMapsScene("hybrid_odd_maps", [], [], cam, dict(sky_enabled=1))


def _raster_setup():
    scene = odd_maps_scene()
    gpu = rr.Renderer(W, H)
    meshes, textures = fw.upload_recorded(scene, gpu, defaults=False)
    view = frame_view(scene, W, H)
    view.num_lights = 0
    assert [t.shape[:2] for t in textures] == [(1, 1), (9, 17), (16, 8), (12, 20), (8, 24), (1, 1)]
    assert meshes[0]["vertices"]["uv"][:, 0].min() == -3.0 and meshes[0]["diffuse_map"] == 2
    return scene, gpu, meshes, textures, view


def test_forward_pass_with_maps_that_are_not_square():
    scene, gpu, meshes, textures, view = _raster_setup()
    gpu.render_forward(view, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    ref = test_gpu_forward._check(gpu, meshes, textures, [], view)
    seen = set(np.unique(ref["visibility"][ref["visibility"] != fw.NONE]))
    tmesh, _ = fw.triangle_of(meshes)
    assert set(int(tmesh[v]) for v in seen) >= {0, 1, 3}, "the floor with the 16 x 8 map and both spheres are in the frame"


def test_rasterised_gbuffer_with_maps_that_are_not_square():
    scene, gpu, meshes, textures, view = _raster_setup()
    gpu.render_hybrid(view, test_gpu_gbuffer_raster.RASTER)
    ref = test_gpu_gbuffer_raster._check(gpu, meshes, textures, view)
    assert (ref["visibility"] != test_gpu_gbuffer_raster.gr.NONE).mean() > 0.3


def test_cast_gbuffer_and_reflections_with_maps_that_are_not_square():
    """the comparisons of test_gpu_hybrid.py: the cast G-buffer's four targets bit for bit, the reflections byte for byte where the ray
    hits and within 1 LSB where it meets the sky"""
    scene = odd_maps_scene()
    gpu = rr.Renderer(W, H)
    meshes = hr.upload_recorded(scene, gpu, False)
    cpu = oa.OracleRenderer(W, H)
    hr.upload_recorded(scene, cpu, False)
    view = hybrid_view(scene, W, H)
    gpu.render_hybrid(view, rr.HYBRID_GBUFFER | rr.HYBRID_RT_REFLECTIONS)
    got = gbuf(gpu)
    ref = hr.gbuffer(cpu, meshes, view, W, H)
    for k in ("position", "normal", "pbr"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(got["albedo"], ref["albedo"])
    hit = got["position"][..., 3] == 1.0
    assert hit.any() and (~hit).any()
    assert len(np.unique(got["albedo"][hit].reshape(-1, 4), axis=0)) > 200, "the albedo target carries the random maps' texels"
    want, kind = hr.reflections(cpu, meshes, got["position"], got["normal"], got["pbr"], view)
    assert_reflections(gpu.read_hybrid(rr.HYBRID_REFLECTIONS), want, kind)
    assert (kind == 1).any() and (kind == 2).any()

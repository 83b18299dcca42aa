"""The cases, terms and shared checks of the tests that hold the rasterised passes to the float64 rasteriser of raster_f64.py:
test_raster_f64_cpu.py (the numpy restatements) and test_gpu_raster_f64.py (the device). It imports no restatement. Not a conftest: test
modules import it.

Each case is there because rasterisers break there: triangles through the near and the far plane, dense slivers, clipped shared edges,
the camera inside a closed cube, geometry beyond the guard band, a grazing floor, vertices and edges exactly on pixel centres, a quad
in the near plane, flipped instances, tiny and odd frames.

The absolute terms of the depth and barycentric envelopes: the largest excess of a restatement over the un-widened five-point envelope,
in float32 ulps of 1.0 (every test prints its own), doubled and rounded up.
  depth         0.75 at fan_and_diagonal (0.61 at soup_300x, 0.59 in the marching-cubes pass, 0 at every other case but the two below):
                DEPTH_ULPS = 2, float32 z / w and the interpolation's roundings.
                huge_floor and huge_floor_fan_in_view have a term of their own: 4,766.39 ulp (2.8e-4) measured at both, so
                HUGE_FLOOR_DEPTH_ULPS = 9,533. Their clip z and w are near 27,000, where float32 steps by 0.002, at vertices that
                weigh about 0.5 in the middle of the frame, where w is about 3: the float32 vertex stage's rounding,
                which a near-plane crossing computed in float64 leaves unchanged. huge_floor_7x5 and the floor's shadow maps measure 0
                and keep the common term.
  barycentrics  3.43 at spokes_behind_the_eye (1.30 and 0.95 at the two huge floors, 0 elsewhere): B_ULPS = 7
The snap's share lies inside the envelope's own width."""
import numpy as np

import raster_f64 as rf
import rust_renderer_amd as rr
from rust_renderer_amd.scenes import Scene, icosphere, quad
from rust_renderer_amd.types import VERTEX_DTYPE

F = np.float32
DEPTH_ULPS = 2
HUGE_FLOOR_DEPTH_ULPS = 9533
B_ULPS = 7
SHADOW_SIZE = 64


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class CaseScene(Scene):
    """parts: [(positions (n, 3), indices, world 3x4 or None)], one mesh each, one white Lambertian material"""
    parts = ()

    def upload(self, renderer):
        white = renderer.default_diffuse_map()
        for pos, idx, world in self.parts:
            v = np.zeros(len(pos), VERTEX_DTYPE)
            v["pos"][:, :3], v["pos"][:, 3] = np.asarray(pos, F), 1.0
            v["normal"][:, :3] = (0.0, 1.0, 0.0)
            v["color"] = 1.0
            renderer.add_mesh(v, np.asarray(idx, np.uint32).reshape(-1), rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.8, 0.8, 1.0), diffuse_map=white), world)
        renderer.initialize_raytracing()
        return renderer


class Recorder:
    """a renderer that only records: every add_mesh as the dict the restatements and raster_f64 read (hybrid_reference.upload_recorded's
    keys), no texture kept, so every map index reads white"""

    def __init__(self):
        self.textures, self.meshes = 0, []

    def default_diffuse_map(self):
        return 0

    def add_texture(self, rgba):
        self.textures += 1
        return self.textures - 1

    def add_mesh(self, vertices, indices, material, world3x4=None):
        w = rr.identity3x4() if world3x4 is None else np.ascontiguousarray(world3x4, dtype=F).reshape(12)
        self.meshes.append(dict(vertices=np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE), indices=np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1),
                                world=w.copy(), diffuse_map=material.diffuse_map, normal_map=material.normal_map,
                                metallic_roughness_map=material.metallic_roughness_map, occlusion_map=material.occlusion_map,
                                base_color=np.array(material.base_color_factor[:3], dtype=F), type=float(material.raytrace_properties[0]),
                                metallic=F(material.metallic_factor), roughness=F(material.roughness_factor)))
        return len(self.meshes) - 1

    def initialize_raytracing(self):
        pass


def make_case(name, parts, eye, target, near, far, W=64, H=48, fov=60.0, exempt=False, depth_ulps=DEPTH_ULPS, excused=0):
    """exempt: a tiny frame, free of the 300-pixel cap; depth_ulps: the case's absolute depth term; excused: how many surely covered
    pixels may show a triangle that is none of the five winners (raster_f64.check_visibility)"""
    scene = CaseScene(name, [], [], rr.camera.Camera(eye, target, fov, W / H, near, far), dict(sky_enabled=1))
    scene.parts = parts
    return dict(name=name, scene=scene, W=W, H=H, exempt=exempt, depth_ulps=depth_ulps, excused=excused)


def case_view(case):
    v = case["scene"].make_view(case["W"], case["H"])
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    v.num_lights = 0
    return v


def soup(seed, n, sigma, spread=6.0, scale=1.0):
    """n triangles: centres uniform in +-spread, vertices normal around them with deviation sigma"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    p = (c + rng.normal(0.0, sigma, (n, 3, 3))) * scale
    return [(p.reshape(-1, 3), np.arange(3 * n), None)]


def grid(origin, eu, ev, n):
    v, i = quad(origin, eu, ev, nu=n, nv=n)
    return [(v["pos"][:, :3].copy(), np.asarray(i).reshape(-1), None)]


def cube():
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = []
    for a, b, cc, d in faces:
        idx += [a, b, cc, a, cc, d]
    return [(c, idx, None)]


def huge_floor(first=0):
    """the +-30,000 floor and a small quad above it; first: which vertex of each floor triangle comes first - it decides which corner the
    fan of a guard-band clipped piece starts at, and so which fan triangle lies in view"""
    o = 30000.0
    p = np.array([(-o, 0.0, o), (o, 0.0, o), (o, 0.0, -o), (-o, 0.0, -o)])
    tri = np.roll(np.array([[0, 1, 2], [0, 2, 3]]), -first, axis=1)
    return [(p, tri.reshape(-1), None)] + grid((-0.5, 0.8, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0), 1)


def spokes(radius=1e6, n=7, centre=(0.3, 0.0, -3.0), phase=0.2):
    """a floor fan around a vertex in view whose rim lies `radius` away, most of it behind the eye: every shared edge runs from a small
    inside end through the near plane to a huge outside end, where a crossing computed from the outside end is off by pixels"""
    a = phase + np.arange(n) * 2.0 * np.pi / n
    rim = np.array(centre) + radius * np.stack([np.cos(a), np.zeros(n), np.sin(a)], -1)
    idx = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    return [(np.concatenate([np.array(centre)[None], rim]), np.array(idx).reshape(-1), None)]


def far_vertex_quad():
    return [(np.array([(-3.0, 0.0, 2.0), (3.0, 0.0, 2.0), (3.0, 0.0, -6.0), (-1e6, 0.0, -1e6)]), [0, 1, 2, 0, 2, 3], None)]


def fan_and_diagonal():
    """in the plane z = 0, one world unit a pixel (see the case): a fan of 64 thin triangles around a vertex on the centre of a pixel, and
    a quad whose shared diagonal runs through pixel centres"""
    a = np.arange(64) * (2.0 * np.pi / 64)
    centre = np.array([-15.5, 0.5, 0.0])
    rim = centre + 12.0 * np.stack([np.cos(a), np.sin(a), np.zeros(64)], -1)
    idx = [[0, 1 + k, 1 + (k + 1) % 64] for k in range(64)]
    q = np.array([(4.5, -9.5, 0.0), (24.5, -9.5, 0.0), (24.5, 10.5, 0.0), (4.5, 10.5, 0.0)])
    return [(np.concatenate([centre[None], rim]), np.array(idx).reshape(-1), None), (q, [0, 1, 2, 0, 2, 3], None)]


def near_plane_tie():
    """a quad lying exactly in the near plane (clip z = 0 at every vertex, in float32 and in float64: near = 0.5 halves exactly), which
    the depth range 0 <= z keeps; its pixels are surely covered and never decided. A farther quad carries the decided pixels."""
    near = np.array([(-0.3, -0.1, -0.5), (-0.1, -0.1, -0.5), (-0.1, 0.1, -0.5), (-0.3, 0.1, -0.5)])
    far = np.array([(0.0, -2.5, -5.0), (4.0, -2.5, -5.0), (4.0, 2.5, -5.0), (0.0, 2.5, -5.0)])
    return [(near, [0, 1, 2, 0, 2, 3], None), (far, [0, 1, 2, 0, 2, 3], None)]


def instances():
    sv, si = icosphere(1)
    rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], F)
    qv, qi = quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), nu=3, nv=3)
    flip = rr.transform3x4((-1.2, 0.8, 1.0), (1.1, 0.2, -0.6), np.array([[0.96, 0.0, -0.28], [0.0, 1.0, 0.0], [0.28, 0.0, 0.96]], F))
    return [(sv["pos"][:, :3].copy(), np.asarray(si).reshape(-1), rr.transform3x4((1.4, 0.6, 0.9), (-1.0, 0.1, 0.0), rot)),
            (qv["pos"][:, :3].copy(), np.asarray(qi).reshape(-1), flip)]


ORIGIN, AHEAD = (0.0, 0.0, 0.0), (0.3, -0.2, -1.0)
FLOOR_EYE, FLOOR_AT = (0.0, 1.0, 0.0), (0.0, 0.2, -4.0)
HUGE_EYE, HUGE_AT = (0.0, 2.0, 3.0), (0.0, 0.5, 0.0)
CASES = {c["name"]: c for c in [
    make_case("soup", soup(1, 40, 2.5), ORIGIN, AHEAD, 0.5, 12.0),                                                        # 1
    make_case("soup_67x41_wide_range", soup(1, 40, 2.5), ORIGIN, AHEAD, 1e-3, 1e5, 67, 41),                               # 2
    make_case("soup_300x", soup(1, 40, 2.5, scale=300.0), ORIGIN, AHEAD, 0.1, 1e4),                                       # 2
    make_case("dense_soup", soup(3, 400, 0.6), ORIGIN, AHEAD, 0.5, 12.0),                                                 # 3
    make_case("floor_through_near", grid((-20.0, 0.0, 20.0), (40.0, 0.0, 0.0), (0.0, 0.0, -40.0), 5), FLOOR_EYE, FLOOR_AT, 0.5, 30.0),   # 4
    make_case("floor_through_far", grid((-20.0, 0.0, 20.0), (40.0, 0.0, 0.0), (0.0, 0.0, -40.0), 5), FLOOR_EYE, FLOOR_AT, 0.5, 9.0),     # 5
    make_case("inside_cube", cube(), (0.2, 0.1, 0.3), (1.0, 0.4, -0.7), 0.05, 10.0),                                      # 6
    make_case("huge_floor", huge_floor(), HUGE_EYE, HUGE_AT, 0.3, 1e5, depth_ulps=HUGE_FLOOR_DEPTH_ULPS),            # 7
    make_case("huge_floor_7x5", huge_floor(), HUGE_EYE, HUGE_AT, 0.3, 1e5, 7, 5, exempt=True),                            # 7
    make_case("huge_floor_fan_in_view", huge_floor(1), HUGE_EYE, HUGE_AT, 0.3, 1e5, depth_ulps=HUGE_FLOOR_DEPTH_ULPS),  # 7
    make_case("spokes_behind_the_eye", spokes(), FLOOR_EYE, FLOOR_AT, 0.5, 30.0),                                         # 4
    make_case("vertex_at_1e6", far_vertex_quad(), HUGE_EYE, HUGE_AT, 0.3, 1e5),                                           # 7
    make_case("grazing_floor", grid((-50.0, 0.0, 50.0), (100.0, 0.0, 0.0), (0.0, 0.0, -100.0), 1), (0.0, 0.02, 0.0), (0.0, 0.0, -1.0), 0.05, 200.0),  # 8
    # fov 90 at distance 24 from the plane z = 0 of a 64 x 48 frame: one world unit is one pixel, (k + 0.5, l + 0.5) a pixel centre
    make_case("fan_and_diagonal", fan_and_diagonal(), (0.0, 0.0, 24.0), (0.0, 0.0, 0.0), 1.0, 100.0, fov=90.0, excused=1),  # 9
    make_case("near_plane_tie", near_plane_tie(), ORIGIN, (0.0, 0.0, -1.0), 0.5, 12.0),                                   # a tie at the near plane
    make_case("instances", instances(), (0.4, 0.9, 3.2), (0.0, 0.1, 0.0), 0.1, 100.0),                                    # 10
    make_case("soup_1x1", soup(1, 40, 2.5), ORIGIN, AHEAD, 0.5, 12.0, 1, 1, exempt=True),                                 # 11
    make_case("soup_257x129", soup(1, 40, 2.5), ORIGIN, AHEAD, 0.5, 12.0, 257, 129),                                      # 11
]}
SHADOW_CASES = ["soup", "dense_soup", "huge_floor"]  # 12: under rr.shadow_cascades of the case's camera and the view's sun

_cache = {}


def recorded(case):
    """the case's meshes as its upload hands them over, without a renderer"""
    r = Recorder()
    case["scene"].upload(r)
    return r.meshes


def prepared(name):
    """a case's meshes, view, truth and records, computed once and shared by the tests of the case"""
    if name not in _cache:
        case = CASES[name]
        meshes = recorded(case)
        view = case_view(case)
        five = rf.five_points(rf.view_matrices(view, meshes), meshes, case["W"], case["H"])
        _cache[name] = dict(case=case, meshes=meshes, view=view, five=five)
    return _cache[name]


def report(name, what, five, **measured):
    print(f"\n{name} [{what}]: {five.counts()} " + " ".join(f"{k}={v:.2f}" for k, v in measured.items()))


# ---- the shadow maps ------------------------------------------------------------------------------------------------------------
def shadow_checks(five, layer, ulps):
    """a cascade's layer (S, S) under the decided / covered rules: decided empty texels hold the clear value, decided covered ones the
    envelope's depth, surely covered ones a fragment no farther than the farthest of the five winners -> the largest depth excess"""
    empty = five.decided & (five.winner < 0)
    assert (layer[empty] == 1.0).all(), f"{int((layer[empty] != 1.0).sum())} decided empty texels were drawn"
    dz = rf.check_depth(five, layer, ulps)
    with np.errstate(invalid="ignore"):  # inf - inf where a point has no winner: not a surely covered texel
        hi = rf.widened(five.d_lo, five.d_hi, ulps)[1]
    holes = five.covered & ~(layer.astype(np.float64) <= hi)
    assert not holes.any(), f"{int(holes.sum())} surely covered texels hold nothing near enough (a crack), first at {tuple(np.argwhere(holes)[0])}"
    return dz


def shadow_truths(case, meshes, params):
    S = SHADOW_SIZE
    return [rf.five_points(rf.clip_matrices(list(params.view_projection_matrices[c]), meshes), meshes, S, S) for c in range(4)]


def shadow_caps(name, fives):
    """the caps on every cascade of a case by itself: at least 300 decided covered texels, at most 15 % undecided"""
    for c, five in enumerate(fives):
        n = five.counts()
        print(f"\n{name} [shadow maps, cascade {c}]: {n}")
        assert n["decided_covered"] >= 300 and n["undecided"] <= 0.15 * n["pixels"], (c, n)


# ---- the marching-cubes pass ----------------------------------------------------------------------------------------------------
MC_W, MC_H, MC_TIME = 64, 48, 5.0


def mc_case():
    """the occluders the pass is seeded by: a floor under the domain [0, 32]^3 and a quad between the camera and the domain"""
    parts = grid((-12.0, -0.5, 44.0), (56.0, 0.0, 0.0), (0.0, 0.0, -56.0), 4) + grid((-8.0, 6.0, 2.0), (8.0, 0.0, -8.0), (0.0, 14.0, 0.0), 2)
    c = make_case("marching_cubes", parts, (-30.0, 28.0, -22.0), (10.0, 15.0, 10.0), 0.1, 1000.0, MC_W, MC_H, fov=30.0)
    c["scene"].view_flags = dict(sky_enabled=1, marching_cubes_enabled=1, time=MC_TIME)
    return c


def mc_checks(five, vis, depth, seed, ulps):
    """visibility under the decision rule; depth at the decided covered pixels in the envelope, the seed's bits where decided hidden"""
    rf.check_visibility(five, vis)
    dz = rf.check_depth(five, depth, ulps)
    hidden = five.decided & (five.winner < 0)
    assert np.array_equal(np.asarray(depth, F)[hidden].view(np.uint32), np.asarray(seed, F)[hidden].view(np.uint32))
    return dz

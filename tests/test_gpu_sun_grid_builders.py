"""-m gpu: the device-built sun grid (csrc/sun_grid_build.hip) held to the host builder (csrc/sun_grid.cpp, itself held to brute force
by tests/cpp/sun_grid_check.cpp) on the geometry that builder is proven on, and the walk (k_trace_sun_grid) held to the tree walk
and to the oracle's brute force with every pixel a probe.

1. builder against builder, bit for bit (uh_sun_grid_compare_builders), over scenes x suns x options (sun_grid_cases.builder_cases);
   a case in which no grid is built stands in REFUSALS with the reason it expects, and the host builder must refuse it too
2. grid, tree walk and brute force on "probe" arrangements - a tessellated floor under the occluders, camera straight down, one
   bounce, sky and lights off -, the walk's variants, and twelve seeded directions of tools/soak_sun_grid.py
3. the grid rebuilt after refits, vertex updates and isosurface updates, under every tree builder, against a fresh context"""
import functools

import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import box, quad
from rust_renderer_amd.types import VERTEX_DTYPE
from sun_grid_cases import PROBE_H, PROBE_SUNS, PROBE_W, SUN, builder_cases, builder_scene, probe_scene, soak_direction
from test_gpu_mesh_deform import DEFORM_WORLD, _rot, _sheet, phase
from test_gpu_mesh_deform import update as update_vertices
from test_gpu_sun_verdicts import WAVEFRONT

pytestmark = pytest.mark.gpu

# ---- 1. builder against builder ---------------------------------------------------------------------------------------------------
CASES = builder_cases()
NO_OCCLUDER = "no triangle can occlude a ray of this direction"  # every triangle is edge-on to the sun (or has no area)
# the cases in which no grid is built, with a part of the reason both builders must give. A case that refuses
# without standing here fails, and so does one that stands here and builds.
REFUSALS = {
    # the torture scene lies in planes z = const: edge-on to every sun without a z component
    "torture-pos_y-defaults": NO_OCCLUDER, "torture-pos_x-defaults": NO_OCCLUDER, "torture-diag_xy-defaults": NO_OCCLUDER, "torture-near_y-defaults": NO_OCCLUDER,
    "torture-neg_y-defaults": NO_OCCLUDER, "torture-neg_x-defaults": NO_OCCLUDER,
    # triangles without area occlude nothing
    "points-up_tilt-defaults": NO_OCCLUDER, "points-neg_y-defaults": NO_OCCLUDER,
    # one plane (z = 0, y = 0 for the sheet; the far scenes' wall is parallel to their grid) that contains the sun direction
    "identical-pos_x-defaults": NO_OCCLUDER, "sheet-pos_x-defaults": NO_OCCLUDER, "one-pos_y-defaults": NO_OCCLUDER, "far_grid-diag_xy-defaults": NO_OCCLUDER,
    "far_grid_at_1000-neg_x-defaults": NO_OCCLUDER,
}
assert 4 * len(REFUSALS) <= len(CASES), "more than a quarter of the matrix refuses: move the geometry or use other suns"
assert set(REFUSALS) <= {c[0] for c in CASES}


def one_frame(r, scene, sun, W=16, H=16):
    loop = rr.FrameLoop(r, scene.make_view(W, H, sun_shadow_enabled=1, sky_enabled=0, lights_enabled=0, num_bounces=1))
    loop.view.sun_dir[:] = list(sun)
    loop.frame(rr.PASS_REFERENCE_PT)


def refusal_of(r):
    """the text after "no sun grid in use" when the context has no grid, None when it has one"""
    try:
        r.sun_grid_compare_builders()
    except UtopianError as e:
        head, sep, reason = str(e).partition("no sun grid in use")
        assert sep, f"the comparison itself failed: {e}"  # e.g. "host builder refused": the builders disagree on whether to refuse
        return reason
    return None


def assert_builders_agree(r, what=""):
    """the part-1 comparison on the grid the context has in use"""
    s = r.get_stats()
    assert s.sun_grid_cells > 0, f"{what}: no grid in use ({refusal_of(r)})"
    d = r.sun_grid_compare_builders()
    print(f"SUNGRID {what}: {d} entries {s.sun_grid_entries} mean list {s.sun_grid_mean_list:.2f}")
    assert d["entries_device"] == d["entries_host"] == s.sun_grid_entries, (what, d)
    assert d["cells_length_differs"] == 0 and d["cells_list_differs"] == 0 and d["cells_cover_differs"] == 0, (what, d)
    assert d["walkable_cells"] > 0, (what, d)
    return d


@pytest.mark.parametrize("case,which,sun_name,options", CASES, ids=[c[0] for c in CASES])
def test_device_builder_equals_host_builder(case, which, sun_name, options):
    scene = builder_scene(which, sun_name if which == "edge_on" else None)
    r = scene.upload(rr.Renderer(16, 16))
    r.set_option("sun_grid_force", 1)
    for k, v in options:
        r.set_option(k, v)
    one_frame(r, scene, SUN[sun_name])
    if r.get_stats().sun_grid_cells > 0:
        assert case not in REFUSALS, "listed as a refusal, but a grid was built"
        assert_builders_agree(r, case)
        return
    reason = refusal_of(r)
    print(f"SUNGRID-REFUSED {case}: {reason}")
    assert reason is not None
    assert case in REFUSALS, f"no grid was built and the case is not listed: {reason}"
    assert REFUSALS[case] in reason, reason
    host = scene.upload(rr.Renderer(16, 16))
    host.set_option("sun_grid_force", 1)
    host.set_option("sun_grid_build", 0)
    for k, v in options:
        host.set_option(k, v)
    one_frame(host, scene, SUN[sun_name])
    host_reason = refusal_of(host)
    assert host.get_stats().sun_grid_cells == 0 and host_reason is not None, "the device builder refuses what the host builder builds"
    assert REFUSALS[case] in host_reason, host_reason


# ---- 2. the walk against brute force --------------------------------------------------------------------------------------------
PROBES = [(a, s) for a in ("torture", "tilted", "soup") for s in ("overhead", "oblique", "oblique_n", "diag_xz")] + [("torture", "near_z"), ("tilted", "low"), ("soup", "tiny")]
# arrangements whose grid cannot answer half of the sun rays itself, with the reason (none)
MOSTLY_TREE = {}


def probe_frames(r, scene, sun, frames=3):
    loop = rr.FrameLoop(r, scene.make_view(PROBE_W, PROBE_H))
    loop.view.sun_dir[:] = list(sun)
    for _ in range(frames):
        loop.frame(rr.PASS_REFERENCE_PT)
    return r.read_accumulation().view(np.uint32), r.get_stats()


@functools.lru_cache(maxsize=None)
def probe_reference(arrangement, sun_name):
    """(scene, the tree walk's accumulation and ray counts), after both have been held to the oracle's brute force"""
    scene = probe_scene(arrangement)
    tree = scene.upload(rr.Renderer(PROBE_W, PROBE_H))
    tree.set_option("sun_grid", 0)
    cpu = scene.upload(oa.OracleRenderer(PROBE_W, PROBE_H, brute_force=True))
    (t, ts), (c, cs) = probe_frames(tree, scene, PROBE_SUNS[sun_name]), probe_frames(cpu, scene, PROBE_SUNS[sun_name])
    assert ts.sun_grid_cells == 0
    assert np.array_equal(t, c), f"tree walk against brute force: {np.count_nonzero(t != c)} words differ"
    assert list(ts.rays)[:4] == list(cs.rays)[:4]
    lit = t.view(np.float32)[..., 0] > 0
    assert lit.any() and not lit.all(), "lit and shadowed pixels must both exist"
    t.setflags(write=False)
    return scene, t, list(ts.rays)


def grid_against_reference(arrangement, sun_name, options=()):
    scene, t, rays = probe_reference(arrangement, sun_name)
    grid = scene.upload(rr.Renderer(PROBE_W, PROBE_H))
    grid.set_option("sun_grid_force", 1)
    for k, v in dict(options).items():
        grid.set_option(k, v)
    g, gs = probe_frames(grid, scene, PROBE_SUNS[sun_name])
    what = f"{arrangement} {sun_name} {dict(options)}"
    assert gs.sun_grid_cells > 0, f"{what}: no grid ({refusal_of(grid)})"
    print(f"SUNGRID-PROBE {what}: {gs.sun_tree_rays} of {gs.rays[rr.RAY_SUN_SHADOW]} sun rays to the tree, {gs.sun_covered_rays} answered by a cover depth, "
          f"{np.count_nonzero(t.view(np.float32)[..., 0] > 0)} of {PROBE_W * PROBE_H} pixels lit")
    assert np.array_equal(g, t), f"{what}: {np.count_nonzero(g != t)} words of the accumulation differ from the tree walk's and brute force's"
    assert list(gs.rays) == rays, what
    assert gs.rays[rr.RAY_SUN_SHADOW] > 0
    if arrangement not in MOSTLY_TREE:
        assert gs.sun_tree_rays * 2 <= gs.rays[rr.RAY_SUN_SHADOW], f"{what}: the grid answered less than half of the sun rays: the case tests the fallback"
    return grid, gs


@pytest.mark.parametrize("arrangement,sun_name", PROBES, ids=[f"{a}-{s}" for a, s in PROBES])
def test_grid_walk_equals_tree_walk_and_brute_force(arrangement, sun_name):
    grid, _ = grid_against_reference(arrangement, sun_name)
    assert_builders_agree(grid, f"probe {arrangement} {sun_name}")


WALK_VARIANTS = {"plain_lists": {"sun_grid_inline_max_mb": 0}, "inline_records": {"sun_grid_inline_max_mb": 8192}, "no_coarse_cover": {"sun_grid_coarse": 0},
                 "coarse_cover_16": {"sun_grid_coarse": 4}, "verdicts_off": {"sun_verdicts": 0}, "verdicts_on": {"sun_verdicts": 1}, "wavefront": WAVEFRONT,
                 "wavefront_verdicts_off": dict(WAVEFRONT, sun_verdicts=0), "counted_visits": {"count_visits": 1}}


@pytest.mark.parametrize("variant", list(WALK_VARIANTS))
@pytest.mark.parametrize("arrangement", ["torture", "tilted"])
def test_walk_variants_on_the_probes(arrangement, variant):
    _, s = grid_against_reference(arrangement, "oblique", WALK_VARIANTS[variant])
    if variant == "counted_visits":
        assert s.shadow_tris_tested > 0 and s.shadow_nodes_visited >= s.rays[rr.RAY_SUN_SHADOW] - s.sun_tree_rays


SOAK_SEEDS = range(1, 13)  # seeds 2, 4, 7 draw a wall edge-on, 3 and 5 an axis, 10 both


@pytest.fixture(scope="module")
def cornell():
    return rr.scenes.cornell_scene(subdivisions=2, tex_size=16)


@pytest.mark.parametrize("seed", SOAK_SEEDS)
def test_soak_directions_grid_equals_tree(cornell, seed):
    """tools/soak_sun_grid.py at a bounded size: its random directions, the grid against the tree walk"""
    W, H = 64, 36
    sun = soak_direction(seed)
    out = []
    for on in (1, 0):
        r = cornell.upload(rr.Renderer(W, H))
        r.set_option("sun_grid", on)
        r.set_option("sun_grid_force", 1)
        loop = rr.FrameLoop(r, cornell.make_view(W, H, sun_shadow_enabled=1, sky_enabled=seed % 2, lights_enabled=0))
        loop.view.sun_dir[:] = list(sun)
        for _ in range(2):
            loop.frame(rr.PASS_REFERENCE_PT)
        out.append((r.read_accumulation().view(np.uint32), r.get_stats(), r))
    (g, gs, grid), (t, ts, _) = out
    print(f"SUNGRID-SOAK seed {seed} sun {sun}: cells {gs.sun_grid_cells}, {gs.sun_tree_rays} of {gs.rays[rr.RAY_SUN_SHADOW]} sun rays to the tree")
    assert gs.sun_grid_cells > 0 and ts.sun_grid_cells == 0, refusal_of(grid)
    assert np.array_equal(g, t), f"{np.count_nonzero(g != t)} words differ"
    assert list(gs.rays) == list(ts.rays) and gs.rays[rr.RAY_SUN_SHADOW] > 0


# ---- 3. the grid that is rebuilt after the geometry changed -----------------------------------------------------------------------
W3, H3 = 64, 48
GROUND, DEFORM, ISO_GROWS, ISO_EMPTIES, BOX = range(5)
ISO_A, ISO_B = (12, 0.0, 32.0), (8, 21.5, 24.5)  # (resolution, lo, hi): A has 320 triangles at time 0 and 452 at time 3; B one at T_ONE, none at time 0
T_ONE = 5.2359877
BOX_WORLD = rr.identity3x4()
MIRRORED = rr.transform3x4((-1.05, 0.9, 1.1), (17.0, 11.0, 14.0), _rot(0.15, 0.5, -0.1))
SCALED = rr.transform3x4((6.0, 0.02, 0.5), (-140.0, 12.0, 4.0))  # the box as a thin plate in the air: 24 x 0.1 x 2


def make_scene3(device_build, sheet_phase=0, t_a=0.0, t_b=T_ONE, deform_world=DEFORM_WORLD, box_world=BOX_WORLD):
    """ground, the deformable sheet of test_gpu_mesh_deform.py, two isosurface meshes, a box: built. An isosurface without triangles is
    a mesh without vertices in its place (what a fresh context can be given directly)"""
    r = rr.Renderer(W3, H3)
    r.set_option("sun_grid_force", 1)  # the sun grid refuses scenes with a ground plane by default
    r.set_option("device_build", device_build)

    def mat(*rgb):
        return rr.make_material(base_color=rgb + (1.0,), diffuse_map=r.default_diffuse_map())

    def isosurface(params, time, material):
        res, lo, hi = params
        count = oa.marching_cubes(res, lo, hi, time=time, order=0, positions=False)["triangles"]
        if count == 0:
            return r.add_mesh(np.zeros(0, VERTEX_DTYPE), np.zeros(0, np.uint32), material), 0
        mesh, tris = r.add_isosurface_mesh(res, lo, hi, time, material=material)
        assert tris == count
        return mesh, tris

    assert r.add_mesh(*quad((-64, 4.99, -64), (0, 0, 160), (160, 0, 0), 8, 8), mat(0.6, 0.6, 0.6)) == GROUND
    assert r.add_mesh(phase(sheet_phase), _sheet()[1], mat(0.8, 0.8, 0.8), deform_world) == DEFORM
    assert isosurface(ISO_A, t_a, mat(0.8, 0.5, 0.3))[0] == ISO_GROWS
    assert isosurface(ISO_B, t_b, mat(0.3, 0.8, 0.4))[0] == ISO_EMPTIES
    assert r.add_mesh(*box((27.0, 7.5, 8.0), (2.0, 2.5, 2.0)), mat(0.2, 0.4, 0.8), box_world) == BOX
    r.build_acceleration()
    return r


def frames3(r, n=3):
    """n frames from a cleared accumulation: after a change of the geometry the first walks the tree, the second rebuilds the grid"""
    r.reset_accumulation()
    r.reset_stats()
    cam = rr.camera.Camera((27.0, 19.0, 33.0), (16.0, 14.0, 16.0), 60.0, W3 / H3, 0.01, 1000.0)
    loop = rr.FrameLoop(r, rr.scenes.Scene("rebuilt", [], [], cam, {}).make_view(W3, H3, sun_shadow_enabled=1, sky_enabled=1, lights_enabled=0))
    for _ in range(n):
        loop.frame(rr.PASS_REFERENCE_PT)
    return r.read_accumulation().view(np.uint32), r.get_stats()


def _transforms(r):
    r.set_instance_transform(DEFORM, MIRRORED)
    r.set_instance_transform(BOX, SCALED)
    r.refit_acceleration()


def _vertices(where):
    def change(r):
        update_vertices(r, phase(1), where, mesh=DEFORM)
        r.refit_acceleration()
    return change


def _isosurface(mesh, params, time):
    def change(r):
        res, lo, hi = params
        assert r.update_isosurface_mesh(mesh, time) == oa.marching_cubes(res, lo, hi, time=time, order=0, positions=False)["triangles"]
        r.build_acceleration()
    return change


# change -> (what is done to the context, the arguments of a fresh context with the final geometry)
CHANGES = {
    "transforms_then_refit": (_transforms, dict(deform_world=MIRRORED, box_world=SCALED)),
    "vertices_from_host": (_vertices("host"), dict(sheet_phase=1)),
    "vertices_from_device": (_vertices("device"), dict(sheet_phase=1)),
    "isosurface_grows": (_isosurface(ISO_GROWS, ISO_A, 3.0), dict(t_a=3.0)),
    "isosurface_empties": (_isosurface(ISO_EMPTIES, ISO_B, 0.0), dict(t_b=0.0)),
}


@pytest.mark.parametrize("device_build", [0, 1, 2])
@pytest.mark.parametrize("change", list(CHANGES))
def test_rebuilt_grid_equals_host_builder_and_a_fresh_context(change, device_build):
    apply, final = CHANGES[change]
    a = make_scene3(device_build)
    before, s0 = frames3(a, 1)
    assert s0.sun_grid_cells > 0, "no grid before the change: a stale one could not show"
    assert_builders_agree(a, f"{change} builder {device_build}, before")
    apply(a)
    after, sa = frames3(a)
    assert_builders_agree(a, f"{change} builder {device_build}, after")
    b = make_scene3(device_build, **final)
    fresh, sb = frames3(b)
    assert sb.sun_grid_cells > 0
    assert np.array_equal(after, fresh), f"{np.count_nonzero(after != fresh)} words differ from the fresh context's"
    assert list(sa.rays) == list(sb.rays) and sa.rays[rr.RAY_SUN_SHADOW] > 0
    assert sa.sun_grid_entries == sb.sun_grid_entries, "the same geometry, the same sun: the same number of entries"

"""CPU: the restatement of the ray-traced glossy reflections (tests/glossy_reference.py) held to float64 quadrature of the BRDF it
estimates, to known answers, and to the adequacy of the gallery scene the GPU tests run on."""
import functools

import numpy as np
import pytest

import glossy_reference as gl
import hybrid_reference as hr
import oracle_api as oa

F = np.float32


# ---- 1. the estimator against float64 quadrature --------------------------------------------------------------------------------------
def quadrature(r, NoV, N):
    """(int D Vis (1 - Fc) NoL dl, int D Vis Fc NoL dl) over the hemisphere in float64: D the GGX distribution with a2 = r^4, Vis
    V_SmithGGXCorrelated (brdf.glsl of Filament's form, 0.5 / (NoL sv + NoV sl)), Fc = (1 - VoH)^5. Midpoint rule on N x N cells of
    (xi, phi), the half vector drawn through the distribution's own CDF - cos^2(theta_h) = (1 - xi) / (1 + (a2 - 1) xi), under which
    D cos(theta_h) dh = dxi dphi / (2 pi) - and dl = 4 VoH dh."""
    a2 = float(r) ** 4
    xi = (np.arange(N) + 0.5) / N
    phi = (np.arange(N) + 0.5) / N * 2.0 * np.pi
    xi, phi = np.meshgrid(xi, phi, indexing="ij")
    c2 = (1.0 - xi) / (1.0 + (a2 - 1.0) * xi)
    ch, sh = np.sqrt(c2), np.sqrt(1.0 - c2)
    h = np.stack([sh * np.cos(phi), sh * np.sin(phi), ch], axis=-1)
    v = np.array([np.sqrt(max(0.0, 1.0 - NoV * NoV)), 0.0, NoV])
    VoH = h @ v
    l = 2.0 * VoH[..., None] * h - v
    NoL = l[..., 2]
    ok = (VoH > 0) & (NoL > 0)
    NoLs = np.where(ok, NoL, 1.0)
    vis = 0.5 / (NoLs * np.sqrt(NoV * NoV * (1.0 - a2) + a2) + NoV * np.sqrt(NoLs * NoLs * (1.0 - a2) + a2))
    Fc = (1.0 - np.where(ok, VoH, 1.0)) ** 5
    w = np.where(ok, vis * NoLs * 4.0 * VoH / ch, 0.0)  # D cos(theta_h) dh is the measure: what is left of D Vis NoL 4 VoH dh
    return float((w * (1.0 - Fc)).mean()), float((w * Fc).mean())


@functools.lru_cache(maxsize=None)
def disk_points_of_a_256_frame():
    return gl._disk_points(256, 256, gl.SEED_XOR)  # frame number 0, s = 0


@pytest.mark.parametrize("NoV", [0.2, 0.6, 1.0])
@pytest.mark.parametrize("r", [0.25, 0.5, 1.0])
def test_the_estimator_integrates_the_brdf(r, NoV):
    t = disk_points_of_a_256_frame()
    n = len(t)
    assert n == 65536
    Nn = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    V = np.tile(np.array([np.sqrt(max(0.0, 1.0 - NoV * NoV)), 0.0, NoV], np.float32), (n, 1))
    s = gl.sample(Nn, V, hr.dot(Nn, V), np.full(n, r, np.float32), t)
    cast = ~s["below"]
    Gw = np.where(cast, s["Gw"], 0).astype(np.float64)
    x5 = np.where(cast, s["x5"], 0).astype(np.float64)
    assert (s["Gw"][cast] >= 0).all() and (s["Gw"][cast] <= 1 + 1e-6).all()
    coarse, fine = quadrature(r, NoV, 512), quadrature(r, NoV, 1024)
    for name, values, a, b in (("scale", Gw * (1.0 - x5), coarse[0], fine[0]), ("bias", Gw * x5, coarse[1], fine[1])):
        quad_err = abs(a - b)  # the step halved: the rule's error at the finer step is no larger than the change
        bound = 5.0 * values.std(ddof=1) / np.sqrt(n) + quad_err
        print(f"r {r} NoV {NoV} {name}: mean {values.mean():.6f} integral {b:.6f} (coarser {a:.6f}) bound {bound:.2e} below {1 - cast.mean():.4f}")
        assert abs(values.mean() - b) <= bound, name


# ---- 2. known answers -------------------------------------------------------------------------------------------------------------------
class Cpu:
    def __init__(self, scene, width=gl.W, height=gl.H, **view):
        self.scene = scene
        self.oracle = oa.OracleRenderer(width, height)
        self.meshes = hr.upload_recorded(scene, self.oracle, True)
        self.view = gl.scene_view(scene, width, height, **view)
        self.g = hr.gbuffer(self.oracle, self.meshes, self.view, width, height)

    def gather(self, furnace=False, order=None, **params):
        self.params = gl.default_params(**params)
        return gl.gather(self.oracle, self.meshes, self.g, self.view, self.params, furnace, order)


def test_at_roughness_zero_every_sample_is_the_mirror_ray_and_weighs_exactly_one():
    """r = 0: alpha = 0, so Ne = normalize3(0, 0, Nh.z) and Hw = Ne.z Nn. Gw is exactly 1: sv = sqrt(NoV NoV) = NoV and sl = NoL, the
    square root of a rounded square returning its operand, and NoL (2 NoV) = 2 (NoL NoV) exactly.
    Hw == Nn bit for bit holds where Nh.z * (1 / sqrt(Nh.z Nh.z)) is exactly 1: normalize3 multiplies by a rounded reciprocal, and
    x * fl(1 / x) is 1 - 2^-24, 1 or 1 + 2^-23. On this floor 83 % of the samples give Hw == Nn bit for bit; every one gives Hw = k Nn
    with k one of those three, and a direction within 4 ulp of the mirror's. Under the furnace the floor (metallic 1, base 1) then
    receives exactly intensity * occlusion at one sample per pixel: (1 - x5) + x5 rounds to 1 for x5 <= 1 / 2."""
    w = Cpu(gl.mirror_floor_scene(), ssao_enabled=0)
    got = w.gather(furnace=True, samples=16, intensity=0.75, blur_radius=0)
    px = got["px"]
    assert len(px["rows"]) > 1000 and (px["r"] == 0).all() and (px["re"] == 0).all()
    ss = gl.samples(w.g, w.view, px, 16)
    with np.errstate(all="ignore"):
        mirror = hr.normalize((F(2.0) * px["NoV"])[:, None] * px["Nn"] - px["V"])
    same = 0
    for s in ss:
        assert not s["below"].any() and (s["Gw"] == 1.0).all()
        k = s["Hw"][:, 1] / px["Nn"][:, 1]  # the floor's normal is (0, 1, 0)
        assert np.isin(k, [F(1.0) - F(2.0 ** -24), F(1.0), F(1.0) + F(2.0 ** -23)]).all() and not s["Hw"][:, [0, 2]].any()
        assert np.abs(s["d"] - mirror).max() <= 4 * 2.0 ** -24
        same += (hr.dot(s["Hw"], s["Hw"]) == 1.0).sum()
    print(f"Hw == Nn bit for bit: {same / (16 * len(px['rows'])):.3f} of the samples")
    assert same > 0.5 * 16 * len(px["rows"])
    assert (got["kind"] == gl.MISSED).all() and got["totals"] == (len(px["rows"]), 16 * len(px["rows"]), 0, 0, 16 * len(px["rows"]))
    # one sample per pixel: the composite adds exactly intensity * occlusion
    got = w.gather(furnace=True, samples=1, intensity=0.75, blur_radius=0)
    Sf, Bf, _ = gl.filter(w.g, got, w.params)
    out, touched = gl.composite(w.g, None, np.zeros((gl.H, gl.W, 4), np.float32), Sf, Bf, w.view, w.meshes, 0.75)
    assert touched.sum() == len(px["rows"]) and np.array_equal(out[touched][:, :3], (F(0.75) * w.g["pbr"][touched][:, 2])[:, None].repeat(3, axis=1))
    assert (w.g["pbr"][touched][:, 2] > 0).all() and not out[~touched].any()


@pytest.mark.parametrize("samples, blur_radius", [(1, 0), (16, 3)])
def test_inside_a_closed_box_every_cast_ray_is_dark(samples, blur_radius):
    w = Cpu(gl.inward_box_scene())
    got = w.gather(samples=samples, blur_radius=blur_radius)
    assert got["cast"].all() and (got["counts"] == (0, samples, 0, 0)).all()
    assert got["totals"][0] == gl.W * gl.H and got["totals"][1] + got["totals"][2] == samples * gl.W * gl.H and got["totals"][4] == 0
    Sf, Bf, _ = gl.filter(w.g, got, w.params)
    assert not Sf[..., :3].any() and not Bf[..., :3].any() and (Sf[..., 3] == 1).all() and (Bf[..., 3] == 1).all()
    before = np.random.default_rng(5).uniform(0, 1, (gl.H, gl.W, 4)).astype(np.float32)
    after, _ = gl.composite(w.g, np.full((gl.H, gl.W), 65535, np.uint16), before, Sf, Bf, w.view, w.meshes, 1.0)
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32)), "the deferred output is the call's without the bit"


def test_the_frames_of_the_chunk_tests_are_adequate():
    """tests/test_gpu_glossy_chunks.py: at one block per CU a grid holds WALK_LANES lanes; the closed box at WALK_BOX_SIZE and 16 samples
    casts between one and eight grids of rays, every one dark; the gallery at WALK_GALLERY_SIZE casts as many sun rays too"""
    Ww, Hh = gl.WALK_BOX_SIZE
    w = Cpu(gl.inward_box_scene(), Ww, Hh)
    got = w.gather(samples=16)
    assert (got["counts"] == (0, 16, 0, 0)).all() and gl.WALK_LANES < got["totals"][1] <= 8 * gl.WALK_LANES and got["totals"][2] > 0
    w = Cpu(gl.gallery_scene(), *gl.WALK_GALLERY_SIZE)
    got = w.gather(samples=16)
    assert gl.WALK_LANES < got["totals"][1] <= 8 * gl.WALK_LANES and gl.WALK_LANES < got["totals"][3] <= 8 * gl.WALK_LANES, "a second grid of sun rays"


def test_an_emissive_wall_brings_the_weights_of_the_samples_that_meet_it():
    w = Cpu(gl.emissive_box_scene())
    got = w.gather(samples=16, max_radiance=0.5, blur_radius=0)
    emit = got["kind"] == gl.EMITTER
    assert emit.sum() > 1000 and not (got["kind"] == gl.MISSED).any() and not (got["kind"] == gl.SUNLIT).any()
    want = (np.where(emit, got["Gw"], 0).astype(np.float64) * min(1.0, 0.5)).sum(axis=1) / 16
    rows = got["px"]["rows"]
    total = (got["S"] + got["Bi"]).reshape(-1, 3)[rows]
    assert np.allclose(total, want[:, None], rtol=1e-5, atol=1e-7)
    assert (got["R"][..., :3][~emit] == 0).all()


def test_the_sums_depend_on_the_order_of_the_samples():
    """samples 0 and 15 exchanged: S of some pixels changes in its last bits, so a device sum in any other order would be caught"""
    w = Cpu(gl.gallery_scene())
    a = w.gather(samples=16)
    order = [15] + list(range(1, 15)) + [0]
    b = w.gather(samples=16, order=order)
    changed = (a["S"].view(np.uint32) != b["S"].view(np.uint32)).any(axis=-1).sum()
    print(f"{changed} pixels of {a['cast'].sum()} change")
    assert changed > 0 and np.allclose(a["S"], b["S"], rtol=1e-5, atol=1e-7)


# ---- 3. the gallery is an adequate fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 16])
def test_the_gallery_has_every_kind_of_pixel_ray_and_tap(samples):
    """Conditions, not measurements, on the oracle's G-buffer at GALLERY_SIZE, 134 x 82, the frame at which tests/test_gpu_glossy.py
    renders the gallery and asserts the same conditions on the device's own G-buffer. (At roughness 0.4 - the largest the scene's set
    {0, 0.15, 0.4, 0.8} leaves under max_roughness - at most 4.5 % of the samples are below at any angle of view: one sample per
    pixel of RTGI's 67 x 41 cannot give 100 of them, so the gallery's frame is that one doubled each way.)"""
    Ww, Hh = gl.GALLERY_SIZE
    w = Cpu(gl.gallery_scene(), Ww, Hh)
    got = w.gather(samples=samples, blur_roughness=gl.GALLERY_BLUR_ROUGHNESS)
    px, p = got["px"], w.params
    kinds = [int(((got["kind"] == k) & ~got["below"]).sum()) for k in range(4)]
    Sf, Bf, info = gl.filter(w.g, got, p, flag=got["counts"][..., gl.MISSED] > 0)
    clean = 1.0 - info["tainted"].sum() / got["cast"].sum()
    print(f"{samples} samples: totals {got['totals']} kinds {kinds} below {got['below'].sum()} rough {px['rough'].sum()} metal {px['metal'].sum()} "
          f"re == 0: {(px['re'] == 0).sum()} re == blur_radius: {(px['re'] == p['blur_radius']).sum()} dropped {info['dropped'].sum()} clean {clean:.3f}")
    assert min(kinds) >= 100, kinds
    assert got["below"].sum() >= 100
    assert px["rough"].sum() >= 100 and px["metal"].sum() >= 100
    assert (px["re"] == 0).sum() >= 100 and (px["re"] == p["blur_radius"]).sum() >= 100
    assert info["dropped"].sum() >= 100
    assert clean >= 0.2
    assert got["totals"][1] + got["totals"][2] == got["totals"][0] * samples
    assert (got["counts"].sum(axis=-1)[got["cast"]] == samples).all() and not got["counts"][~got["cast"]].any()
    roughness = {float(m["roughness"]) for m in w.meshes}
    assert {0.0, F(0.15), F(0.4), F(0.8)} <= {F(x) for x in roughness} and {float(m["metallic"]) for m in w.meshes} == {0.0, 1.0}

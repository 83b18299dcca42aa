"""CPU: the float64 reading of tests/hybrid_f64.py against the float32 restatements of tests/hybrid_frame_reference.py and
tests/ibl_reference.py, on synthetic G-buffers of random values and of the value edges (metallic and roughness 0 and 1, factors 0, 1
and 1.5, occlusion 0, black and white albedo, normals facing away from the eye, lights behind the surface, a spot exponent of 0). The
restatements are what the device is held to in ulp; this pins them to an evaluation written independently from the shaders. The
reading's calculateShadow interval and reservoir term are held to the composed restatement (tests/hybrid_compose_reference.py) on the
oracle's G-buffer and reservoirs and the numpy shadow maps, where the interval's ambiguous share is established too."""
import numpy as np
import pytest

import hybrid_compose_reference as cr
import hybrid_f64 as hf
import hybrid_frame_reference as fr
import ibl_reference as ir
import rust_renderer_amd as rr
import shadow_map_reference as sr
from hybrid_util import cast_planes, frame_view, plane_view
from test_hybrid_compose_cpu import H as CH, W as CW, build_world

F = np.float32
W, H = 48, 36


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


MESHES = [dict(metallic=F(m), roughness=F(r), base_color=np.array(bc, F), type=t)
          for m, r, bc, t in ((1.0, 1.0, (1.0, 1.0, 1.0), 0.0), (0.0, 0.0, (0.9, 0.5, 0.2), 1.0), (1.5, 1.5, (0.3, 0.8, 1.0), 0.0),
                              (1.0, 0.5, (1.0, 1.0, 1.0), 1.0), (0.5, 1.5, (0.0, 0.0, 0.0), 0.0))]


def synthetic_gbuffer(seed, eye, edges):
    """(H, W) G-buffer around the origin seen from eye; `edges`: every pixel takes its metallic / roughness / occlusion / albedo from
    {0, 1} and a third of the normals face away from the eye or graze it"""
    rng = np.random.default_rng(seed)
    n = H * W
    P = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    N = _unit(rng.normal(size=(n, 3)))
    if edges:
        V = _unit(np.asarray(eye, np.float64)[None, :] - P)
        kind = np.arange(n) % 3
        away = _unit(-V + 0.3 * N)  # N.V < 0: NdotV clamps to 0
        side = _unit(np.cross(V, N))  # perpendicular to V: N.V within an ulp of 0
        N = np.where((kind == 1)[:, None], away, np.where((kind == 2)[:, None], side, N))
        pbr = np.stack([rng.integers(0, 2, n), rng.integers(0, 2, n), rng.integers(0, 2, n), rng.integers(0, len(MESHES) + 1, n)], -1).astype(F)
        alb = (rng.integers(0, 2, (n, 3)) * 255).astype(np.uint8)
    else:
        pbr = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.integers(0, len(MESHES), (n, 1))], -1).astype(F)
        alb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    g = dict(position=np.concatenate([P, np.ones((n, 1), F)], -1).reshape(H, W, 4), normal=np.concatenate([N, np.ones((n, 1), F)], -1).reshape(H, W, 4),
             albedo=np.concatenate([alb, np.full((n, 1), 255, np.uint8)], -1).reshape(H, W, 4), pbr=pbr.reshape(H, W, 4))
    return g, rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W, 4)).astype(np.uint8), rng.integers(0, 65536, (H, W)).astype(np.uint16)


def lights_of_every_kind(seed, n=8):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        l = rr.make_light(tuple(rng.uniform(-3.0, 3.0, 3)), color=tuple(rng.uniform(0.2, 1.0, 3)))
        l.light_type = float((0, 1, 2, 5)[k % 4])
        l.attenuation[:] = tuple(rng.uniform((0.5, 0.0, 0.05), (1.0, 0.3, 0.4)))
        l.direction[:] = tuple(rng.uniform(-1.0, 1.0, 3))
        l.spot = 0.0 if k == 2 else float(rng.uniform(1.0, 16.0))  # light 2: a spot light with exponent 0
        out.append(l)
    return out


def view_for(eye, rt, ssao, n_lights):
    v = plane_view(eye, (0.0, 0.0, 0.0), W, H)
    v.eye_pos[:] = eye
    v.sun_dir[:] = (0.3, 0.8, -0.5)
    v.raytracing_supported, v.ssao_enabled, v.num_lights = rt, ssao, n_lights
    return v


def check_deferred(got32, want, scale, sens, kappa, where):
    """the restatement's float32 output against the float64 reading within deferred_bound; returns the worst error in units of the
    bound"""
    g = got32[..., :3].astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(g), fin), f"{where}: non-finite patterns differ"
    err = np.where(fin, np.abs(g - np.where(fin, want, 0.0)), 0.0)
    bound = hf.deferred_bound(scale, sens, kappa)
    worst = hf.worst_ratio(err, bound)
    assert worst <= 1.0, f"{where}: error {worst:.3g} x the bound"
    return worst


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("rt,ssao", [(0, 0), (1, 1)])
def test_deferred_reading_holds_the_restatement(edges, rt, ssao):
    eye = (0.5, 3.0, 4.0)
    g, sh, refl, ss = synthetic_gbuffer(7 + edges, eye, edges)
    lights = lights_of_every_kind(3)
    v = view_for(eye, rt, ssao, len(lights))
    want, scale, sens, kappa = hf.deferred(g, sh, refl, ss, v, MESHES, lights)
    check_deferred(fr.deferred(g, sh, refl, ss, v, MESHES, lights), want, scale, sens, kappa, f"edges={edges}")
    assert (kappa > hf.KAPPA_WELL).any() and (kappa <= hf.KAPPA_WELL).mean() > 0.5, "both tiers are reached"


def test_the_ggx_term_at_roughness_zero_and_n_equal_h_is_nan_in_both():
    """roughness 0 and N = V = L exactly: a2 = 0 and dn = NdotH^2 (0 - 1) + 1 = 0, so NDF = 0 / 0 - the GLSL's own NaN; both readings
    give NaN in every channel, and a roughness of 0 elsewhere gives a finite pixel"""
    v = view_for((0.0, 5.0, 0.0), 0, 0, 0)
    v.sun_dir[:] = (0.0, 1.0, 0.0)
    g = dict(position=np.array([[[0, 0, 0, 1], [1, 0, 0, 1]]], F), normal=np.array([[[0, 1, 0, 1], [0, 1, 0, 1]]], F),
             albedo=np.full((1, 2, 4), 255, np.uint8), pbr=np.array([[[0, 0, 1, 0], [0, 0, 1, 0]]], F))
    meshes = [dict(metallic=F(1), roughness=F(1), base_color=np.ones(3, F), type=0.0)]
    args = (g, np.zeros((1, 2), np.uint8), np.zeros((1, 2, 4), np.uint8), np.zeros((1, 2), np.uint16), v, meshes, [])
    got, (want, scale, sens, kappa) = fr.deferred(*args), hf.deferred(*args)
    assert np.isnan(got[0, 0, :3]).all() and np.isnan(want[0, 0]).all()
    assert np.isfinite(got[0, 1, :3]).all() and np.isfinite(want[0, 1]).all()


def smooth_maps(seed):
    """IBL maps of smooth functions of the texel direction (as the device's are: the sky), and a smooth LUT, in the device's layouts"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.2, 1.0, (3, 3))

    def cube(S, shift):
        out = np.ones((6, S, S, 4), F)
        jj, ii = np.mgrid[0:S, 0:S]
        for f in range(6):
            d = ir.texel_dir(f, ii.reshape(-1), jj.reshape(-1), S).astype(np.float64)
            out[f, ..., :3] = (0.6 + 0.4 * np.sin(d @ a + shift)).reshape(S, S, 3)
        return out

    y, x = np.mgrid[0:512, 0:512] / 512.0
    lut = np.stack([0.2 + 0.7 * x * (1 - 0.5 * y), 0.05 + 0.1 * y * (1 - x)], -1).astype(np.float16)
    return dict(irr=cube(512, 0.0), spec=[cube(512 >> m, 0.1 * m) for m in range(8)], lut=lut)


@pytest.fixture(scope="module")
def maps():
    return smooth_maps(5)


@pytest.mark.parametrize("edges", [False, True])
def test_deferred_with_ibl_reading_holds_the_restatement(maps, edges):
    """imageBasedLighting through both readers' own cube, lod and LUT samplers. The edges reach lod 7 and its clamp (roughness 1 and
    1.5), LUT v = 0 and v < 0 through the mirror (roughness 1, 1.5) and LUT u = 0 (NdotV = 0)"""
    eye = (0.5, 3.0, 4.0)
    g, sh, refl, ss = synthetic_gbuffer(11 + edges, eye, edges)
    lights = lights_of_every_kind(4)
    v = view_for(eye, 1, 1, len(lights))
    v.ibl_enabled = 1
    want, scale, sens, kappa = hf.deferred(g, sh, refl, ss, v, MESHES, lights, maps)
    check_deferred(ir.deferred_ibl(g, sh, refl, ss, v, MESHES, lights, maps), want, scale, sens, kappa, f"ibl edges={edges}")
    if edges:
        r = g["pbr"][..., 1] * np.array([m["roughness"] for m in MESHES] + [1.0], F)[g["pbr"][..., 3].astype(int)]
        assert (r == 0).any() and (r == 1).any() and (r > 1).any()


def test_the_lut_reading_mirrors_below_v_zero():
    lut = smooth_maps(5)["lut"]
    u = np.array([0.3, 0.3, 0.0])
    got = hf.lut_lookup(lut, u, np.array([-0.25 / 512, 0.25 / 512, 0.5]))
    assert np.array_equal(got[0], got[1]), "v = -a reads what v = +a reads within the first half texel"
    want = ir.lut_bilinear(lut, u.astype(F), np.array([-0.25 / 512, 0.25 / 512, 0.5], F))
    assert np.allclose(got, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("S", [4, 8, 512])
def test_cube_reading_equals_the_restatement_at_edges_and_corners(maps, S):
    """every texel of a level read at directions that straddle the face edges and corners: the seamless fold and the corner rule"""
    level = maps["spec"][{4: 7, 8: 6, 512: 0}[S]]
    rng = np.random.default_rng(S)
    d = rng.normal(size=(4000, 3))
    d[:1000] = np.sign(d[:1000]) * np.maximum(np.abs(d[:1000]), 1.0)  # near the corners: |x| ~ |y| ~ |z|
    d[1000:2000, 1] = d[1000:2000, 0] * (1 + 1e-3 * rng.normal(size=1000))  # near an edge
    d = d.astype(F)
    got = hf.cube_bilinear(level, d.astype(np.float64))
    want = ir.cube_bilinear(level, d)
    assert np.allclose(got, want, rtol=2e-6, atol=0)


def test_ssao_interval_holds_the_restatement():
    """the corner of two planes and a flat wall: the restatement's texels lie in the float64 interval, and the interval is narrow"""
    view = plane_view((0.0, 0.2, 0.0), (0.0, -0.6, -2.0), W, H)
    pos, nrm = cast_planes(view, [((0.0, -0.5, 0.0), np.array([0.0, 1.0, 0.0])), ((0.0, 0.0, -2.0), np.array([0.0, 0.0, 1.0]))], W, H)
    got = fr.ssao(pos, nrm, view).astype(np.int64)
    lo, hi = hf.ssao(pos, nrm, view)
    assert ((lo <= got) & (got <= hi)).all(), np.count_nonzero((got < lo) | (got > hi))
    assert (got < 65535).any() and np.median(hi - lo) <= 1
    rows = np.array([0, 17, H - 1])
    lo2, hi2 = hf.ssao(pos, nrm, view, rows)
    assert np.array_equal(lo2, lo[rows]) and np.array_equal(hi2, hi[rows])


def test_present_reading_is_within_one_lsb_of_the_restatement():
    rng = np.random.default_rng(2)
    img = np.ones((H, W, 4), F)
    img[..., :3] = rng.choice([0.0, 1e-4, 0.0031308, 0.5, 1.0, 1.5, -0.2, np.nan, np.inf], (H, W, 3)) * rng.uniform(0.5, 1.0, (H, W, 3))
    img[: H // 2, :, :3] = rng.uniform(0.0, 1.0, (H // 2, W, 3))
    _, want = hf.present(img)
    got = fr.present(img, fxaa_enabled=False)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


# ---- calculateShadow and the reservoir term ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    return build_world()


def test_shadow_factor_interval_holds_the_restatement_and_is_mostly_single_valued(world):
    """on the oracle's G-buffer of the tightened synthetic scene and the numpy shadow maps at 256: the float32 restatement's factor lies
    inside the float64 interval at every pixel; at most a quarter of the geometry pixels have an interval that is not a single value,
    and the single-valued ones are both fully lit and shadowed"""
    g, (params, maps) = world["g"], world["shadow"]
    v = frame_view(world["scene"], CW, CH)
    P = g["position"][..., :3].reshape(-1, 3)
    geo = (g["position"][..., 3] != 0).reshape(-1)
    lo, hi, c_lo, c_hi = hf.shadow_interval(P, v, params, maps)
    factor, cascade = sr.calculate_shadow(P.astype(F), v, params, maps)
    slack = 16 * hf.ULP  # the float32 sum of nine taps and its division by 9
    assert ((lo - slack <= factor) & (factor <= hi + slack))[geo].all(), np.count_nonzero(~((lo - slack <= factor) & (factor <= hi + slack))[geo])
    assert ((c_lo <= cascade) & (cascade <= c_hi))[geo].all()
    single = lo == hi
    share = 1.0 - single[geo].mean()
    print(f"ambiguous share {share:.4f} of {geo.sum()} geometry pixels; two cascades possible at {(c_lo != c_hi)[geo].sum()}")
    assert share <= 0.25, share
    assert (single & geo & (hi == 1.0)).any() and (single & geo & (hi < 1.0)).any()
    assert set(np.unique(c_lo[geo])) == {0, 1, 2, 3}


@pytest.mark.parametrize("rt", [1, 0])
@pytest.mark.parametrize("ibl", [0, 1])
def test_deferred_reading_with_shadow_maps_and_reservoirs_holds_the_composed_restatement(world, maps, ibl, rt):
    """rt = 0: no reflection mix, so the reservoir light's term shows on the metal floor too, where nearly all arrived rays start (the
    lights stand behind the occluders)"""
    g, sh, refl, ss, meshes, lights = (world[k] for k in ("g", "sh", "refl", "ss", "meshes", "lights"))
    geo = g["position"][..., 3] != 0
    for kw in (dict(shadow=world["shadow"]), dict(res=world["res"], vis=world["vis"]), dict(shadow=world["shadow"], res=world["res"], vis=world["vis"])):
        v = frame_view(world["scene"], CW, CH, raytracing_supported=rt)
        v.num_lights, v.ibl_enabled, v.shadows_enabled = len(lights), ibl, int("shadow" in kw)
        m = maps if ibl else None
        want, scale, sens, kappa = hf.deferred(g, sh, refl, ss, v, meshes, lights, m, **kw)
        got = cr.deferred(g, sh, refl, ss, v, meshes, lights, maps=m, **kw)[..., :3].astype(np.float64)
        assert np.isfinite(got[geo]).all() and np.isfinite(want[..., geo, :]).all()
        err, bound = hf.interval_error(got, want, scale, sens, kappa)
        worst = hf.worst_ratio(err[geo], bound[geo])
        assert worst <= 1.0, (ibl, rt, sorted(kw), worst)
        if "res" in kw and rt == 0:  # the bound notices the term: on 20 pixels at least the sun-only frame lies a hundred bounds away
            v0 = frame_view(world["scene"], CW, CH, raytracing_supported=rt)
            v0.num_lights, v0.ibl_enabled, v0.shadows_enabled = 0, ibl, v.shadows_enabled
            sun = cr.deferred(g, sh, refl, ss, v0, meshes, [], maps=m, **{k: x for k, x in kw.items() if k == "shadow"})[..., :3].astype(np.float64)
            arrived = geo & (world["vis"] == 255)
            e, b = hf.interval_error(sun, want, scale, sens, kappa)
            assert (e[arrived].max(axis=-1) > 100.0 * b[arrived].max(axis=-1)).sum() >= 20

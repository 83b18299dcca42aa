"""GPU: the device's SSAO, deferred and present passes against the float64 reading of tests/hybrid_f64.py, on the device's own inputs
(cornell, spheres and the synthetic scene; 1,024 lights on sampled rows at 1080p; IBL off and on; the deferred variants that combine IBL,
shadow maps and reservoir lights at 97 x 61), and a scene of value edges - constant
metallic / roughness / occlusion maps of 0 and 255, factors 0, 1 and 1.5, black and white albedo, normals facing away from the eye, a
spot light of exponent 0 and a light behind the surface - against both the float32 restatements and the float64 reading."""
import numpy as np
import pytest

import hybrid_f64 as hf
import hybrid_frame_reference as fr
import hybrid_reference as hr
import ibl_reference as ir
import rust_renderer_amd as rr
from hybrid_util import (CONSUMER_ULP, DEFERRED_ULP, W, H, SyntheticScene, add_lights, assets, frame_view, gbuf, ibl_view, pair,  # noqa: F401
                         record, scene_named, ulps)
from rust_renderer_amd.scenes import quad
from test_gpu_deferred_variants import build_variants, front_lights

pytestmark = pytest.mark.gpu


def check_f64(gpu, view, meshes, lights, maps, name, rows=None, shadow=None, res=None, vis=None):
    """the device's images of the last UH_HYBRID_FRAME call against the float64 reading (deferred on the geometry pixels, SSAO inside
    its interval, present within 1 LSB with FXAA off); rows: only these rows (deferred / present) and SSAO texel rows. shadow: the
    device's (params, maps) - the factor is then an interval, at most a quarter of the geometry pixels may have more than one value in
    it, and the others must be both lit and shadowed; res, vis: the spatial reservoirs and the light-visibility image of the call"""
    g, d = gbuf(gpu), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    sh, refl, ss = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE)
    Hh = g["position"].shape[0]
    sel = np.arange(Hh) if rows is None else np.asarray(rows)
    sub = {k: v[sel] for k, v in g.items()}
    want, scale, sens, kappa = hf.deferred(sub, sh[sel], refl[sel], ss[::-1][sel][::-1], view, meshes, lights, maps, shadow,
                                           None if res is None else res[sel], None if vis is None else vis[sel])
    geo = sub["position"][..., 3] == 1.0
    got = d[sel][..., :3].astype(np.float64)
    fin = np.isfinite(want).reshape((-1,) + got.shape).all(axis=0) & geo[..., None]
    assert np.array_equal(np.isfinite(got) & geo[..., None], fin), f"{name}: non-finite pattern"
    err, bound = hf.interval_error(np.where(fin, got, 0.0), np.where(fin, want, 0.0), scale, sens, kappa)
    err = np.where(fin, err, 0.0)
    ratio = hf.worst_ratio(err, bound)
    ambiguous = 0.0
    if shadow is not None:
        lo, hi = hf.shadow_interval(sub["position"][..., :3].reshape(-1, 3), view, *shadow)[:2]
        single, flat = lo == hi, geo.reshape(-1)
        ambiguous = float(1.0 - single[flat].mean())
        assert ambiguous <= 0.25, f"{name}: the shadow factor is an interval at {ambiguous:.3f} of the geometry pixels"
        assert (single & flat & (hi == 1.0)).any() and (single & flat & (hi < 1.0)).any(), f"{name}: lit and shadowed single-valued pixels"
    scale = scale.reshape((-1,) + got.shape)[-1]
    well = geo & (kappa <= hf.KAPPA_WELL)
    rel = lambda m: hf.worst_ratio(np.where(m[..., None], err, 0.0), scale) / hf.ULP
    peak = geo & (kappa > hf.KAPPA_WELL)
    # SSAO: inside the float64 interval at every texel
    lo, hi = hf.ssao(g["position"], g["normal"], view, sel)
    s = ss[sel].astype(np.int64)
    outside = int(np.count_nonzero((s < lo) | (s > hi)))
    # present (the caller ran with FXAA off)
    _, p64 = hf.present(d)
    lsb = int(np.abs(gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)[sel].astype(int) - p64[sel].astype(int)).max())
    record("hybrid_frame", f"f64-{name}", deferred_worst_of_bound=round(ratio, 4), well_max_ulp_of_scale=round(rel(well), 2), peak_pixels=int(peak.sum()),
           peak_max_ulp_of_scale=round(rel(peak), 2), shadow_ambiguous_share=round(ambiguous, 4), ssao_outside=outside, ssao_median_width=float(np.median(hi - lo)), present_max_lsb=lsb)
    assert geo.any() and ratio <= 1.0, f"{name}: deferred error {ratio:.3g} x the bound"
    assert outside == 0, f"{name}: {outside} SSAO texels outside the interval"
    assert lsb <= 1, f"{name}: present {lsb} LSB"
    return g, d


@pytest.mark.parametrize("ibl", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "spheres", "synthetic"])
def test_the_device_against_the_float64_reading(assets, name, ibl):
    scene = scene_named(name, assets)
    gpu, cpu, meshes = pair(scene)
    lights = add_lights(gpu, 12, 9, (0, 1, 2, 5)) if name == "synthetic" else []
    v = ibl_view(scene, fxaa_enabled=0) if ibl else frame_view(scene, fxaa_enabled=0)
    v.num_lights = len(lights)
    maps = None
    if ibl:
        gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_ENVIRONMENT)
        maps = ir.read_maps(gpu)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    check_f64(gpu, v, meshes, lights, maps, f"{name}-ibl{ibl}")


@pytest.fixture(scope="module")
def together():
    """the second world of tests/test_gpu_deferred_variants.py: the tightened synthetic scene at 97 x 61, 8 lights on the camera's side
    (the reservoir light's term shows on the matte meshes), three reservoir frames, shadow maps of size 256 and the IBL maps"""
    return build_variants(front_lights())


@pytest.mark.parametrize("ibl, shadows, restir", [(1, 1, 0), (0, 1, 1), (1, 1, 1)])
def test_the_device_against_the_float64_reading_with_the_features_together(together, ibl, shadows, restir):
    """k_hybrid_deferred<kIbl, kShadow, kRestir> for the triples that combine features, against the reading's calculateShadow interval
    and reservoir term"""
    w, gpu = together, together.gpu
    v = w.view(ibl=ibl, shadows=shadows, fxaa_enabled=0)
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(v, rr.HYBRID_FRAME | (rr.HYBRID_RESTIR_LIGHTS if restir else 0))
    res, vis = (gpu.read_reservoirs(2), gpu.read_hybrid(rr.HYBRID_LIGHT_VISIBILITY)) if restir else (None, None)
    if restir:
        matte = np.array([m["type"] for m in w.meshes], np.float32)[gpu.read_hybrid(rr.HYBRID_PBR)[..., 3].astype(int) % len(w.meshes)] != 1.0
        assert ((vis == 255) & matte).sum() >= 100, "the reservoir light's term shows"
    check_f64(gpu, v, w.meshes, w.all_lights(), w.maps if ibl else None, f"synthetic-97x61-ibl{ibl}-shadow{shadows}-restir{restir}",
              shadow=w.shadow if shadows else None, res=res, vis=vis)


@pytest.mark.parametrize("ibl", [0, 1])
def test_1024_lights_at_1080p_against_the_float64_reading_on_sampled_rows(ibl):
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    Wf, Hf = 1920, 1080
    gpu = rr.Renderer(Wf, Hf)
    meshes = hr.upload_recorded(scene, gpu, defaults=False)
    lights = add_lights(gpu, 1024, 11, (1, 2))
    v = ibl_view(scene, Wf, Hf, fxaa_enabled=0) if ibl else frame_view(scene, Wf, Hf, fxaa_enabled=0)
    v.num_lights = 1024
    maps = None
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | (rr.HYBRID_ENVIRONMENT if ibl else 0))
    if ibl:
        maps = ir.read_maps(gpu)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    check_f64(gpu, v, meshes, lights, maps, f"1080p-1024-lights-ibl{ibl}", rows=[0, 217, 540, 811, 1079])


# ---- C. value edges -----------------------------------------------------------------------------------------------------------------
def _flat_quad(origin, eu, ev, tangent=(0.0, 0.0, 0.0)):
    v, i = quad(origin, eu, ev, nu=1, nv=1)
    v["tangent"][:, :3] = tangent
    return v, i


class EdgeScene(SyntheticScene):
    """a wall of 12 x 12 quads facing the camera, one material each: metallic-roughness maps of 0 / 255 in b (metallic) and g
    (roughness), occlusion 0 / 255, a black or white diffuse map, and metallic / roughness factors of 0, 1 and 1.5; then a quad with
    base_color 0, a quad whose normal map points into the surface (N.V < 0), and a quad seen edge-on below the wall (N.V ~ 0). Every
    fourth quad is metal."""

    def upload(self, renderer):
        renderer.default_diffuse_map()
        const = lambda rgba: renderer.add_texture(np.tile(np.array(rgba, np.uint8), (4, 4, 1)))
        diffuse = [const((0, 0, 0, 255)), const((255, 255, 255, 255))]
        mr = {(m, r): const((0, r, m, 255)) for m in (0, 255) for r in (0, 255)}
        occ = [const((0, 0, 0, 255)), const((255, 255, 255, 255))]
        flat, inward = const((128, 128, 255, 255)), const((128, 128, 0, 255))
        factors = (0.0, 1.0, 1.5)
        k = 0
        for (m, r), tex in mr.items():
            for o in (0, 1):
                for b in (0, 1):
                    for mf in factors:
                        for rf in factors:
                            x, y = k % 12, k // 12
                            mat = rr.make_material(rr.METAL if k % 4 == 3 else rr.LAMBERTIAN, 0.0, (1.0, 1.0, 1.0, 1.0), diffuse_map=diffuse[b],
                                                   metallic=mf, roughness=rf)
                            mat.normal_map, mat.metallic_roughness_map, mat.occlusion_map = flat, tex, occ[o]
                            renderer.add_mesh(*_flat_quad((-3.3 + 0.55 * x, -3.3 + 0.55 * y, 0.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)), mat)
                            k += 1
        extra = [((0.0, 0.0, 0.0, 1.0), flat, (0.0, 0.0, 0.0), ((3.5, -1.0, 0.0), (1.5, 0.0, 0.0), (0.0, 1.5, 0.0))),
                 ((1.0, 1.0, 1.0, 1.0), inward, (1.0, 0.0, 0.0), ((3.5, 1.0, 0.0), (1.5, 0.0, 0.0), (0.0, 1.5, 0.0))),
                 ((1.0, 1.0, 1.0, 1.0), flat, (0.0, 0.0, 0.0), ((-3.3, -3.6, 3.0), (6.6, 0.0, 0.0), (0.0, 0.0, -3.0)))]
        for base, nmap, tangent, (o, eu, ev) in extra:
            mat = rr.make_material(rr.LAMBERTIAN, 0.0, base, diffuse_map=diffuse[1], metallic=1.0, roughness=0.5)
            mat.normal_map, mat.metallic_roughness_map, mat.occlusion_map = nmap, mr[(255, 255)], occ[1]
            renderer.add_mesh(*_flat_quad(o, eu, ev, tangent), mat)
        renderer.initialize_raytracing()
        return renderer


def edge_scene():
    # the eye level with the edge-on quad's plane (y = -3.6 is below the eye; the quad is seen at a grazing angle)
    cam = rr.camera.Camera((0.3, -3.2, 8.0), (0.3, -0.2, 0.0), 60.0, W / H, 0.01, 1000.0)
    return EdgeScene("value_edges", [], [], cam, dict(sky_enabled=1))


def edge_lights(gpu):
    """a spot light of exponent 0 aimed away from the wall (pow(0, 0) = 1 wherever dot(L, dir) <= 0), a point light behind the wall,
    a point light in front, a directional light"""
    out = []
    for pos, typ, direction, spot in (((0.0, 0.0, 3.0), 2.0, (0.0, 0.0, 1.0), 0.0), ((0.0, 0.0, -2.0), 1.0, (0.0, 0.0, 0.0), 1.0),
                                      ((1.0, 2.0, 2.0), 1.0, (0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 0.0), 0.0, (0.3, -0.5, 1.0), 1.0)):
        l = rr.make_light(pos, color=(0.9, 0.8, 0.7))
        l.light_type, l.spot = typ, spot
        l.direction[:] = direction
        l.attenuation[:] = (1.0, 0.1, 0.05)
        gpu.add_gpu_light(l)
        out.append(l)
    gpu.initialize_raytracing()
    return out


@pytest.mark.parametrize("ibl", [0, 1])
def test_value_edges_against_the_restatement_and_the_float64_reading(ibl):
    """Non-finite values: deferred.frag's own arithmetic gives NaN where roughness is 0 and NdotH is exactly 1 (NDF = 0 / 0); the
    device's non-finite pattern must equal the restatement's wherever that happens (on this view no pixel meets it exactly, and the
    pattern is then all-finite). Roughness 1.5 reaches cube lod 10.5 (clamped to 7) and the LUT at v = -0.5 (mirrored); roughness 0
    reaches lod 0 and v = 1; N.V <= 0 reaches the LUT at u = 0."""
    scene = edge_scene()
    gpu, cpu, meshes = pair(scene)
    lights = edge_lights(gpu)
    v = ibl_view(scene, fxaa_enabled=0) if ibl else frame_view(scene, fxaa_enabled=0)
    v.num_lights = len(lights)
    maps = None
    if ibl:
        gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_ENVIRONMENT)
        maps = ir.read_maps(gpu)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    g, d = gbuf(gpu), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    sh, refl, ss = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE)
    geo = g["position"][..., 3] == 1.0
    # the edges are on screen
    mf = np.array([m["metallic"] for m in meshes], np.float32)[g["pbr"][..., 3].astype(int)[geo]]
    rough = g["pbr"][..., 1][geo] * np.array([m["roughness"] for m in meshes], np.float32)[g["pbr"][..., 3].astype(int)[geo]]
    V = np.array(v.eye_pos[:], np.float32) - g["position"][..., :3][geo]
    ndv = np.sum(g["normal"][..., :3][geo] * V, axis=-1)
    assert (rough == 0).any() and (rough == 1).any() and (rough == 1.5).any() and (mf == 1.5).any()
    assert (g["pbr"][..., 2][geo] == 0).any() and (ndv < 0).any(), "occlusion 0 and normals facing away"
    ref = ir.deferred_ibl(g, sh, refl, ss, v, meshes, lights, maps) if ibl else fr.deferred(g, sh, refl, ss, v, meshes, lights)
    fin = np.isfinite(ref[geo])
    assert np.array_equal(np.isfinite(d[geo]), fin), "non-finite patterns"
    u = ulps(d[geo][fin], ref[geo][fin])
    record("hybrid_frame", f"edges-ibl{ibl}", restatement_max_ulp=int(u.max()), nonfinite=int((~fin).sum()))
    assert u.max() <= (CONSUMER_ULP if ibl else DEFERRED_ULP), u.max()
    check_f64(gpu, v, meshes, lights, maps, f"edges-ibl{ibl}")

"""GPU: the IBL maps (uh_render_hybrid's UH_HYBRID_ENVIRONMENT) and their consumers against the CPU reference of tests/ibl_reference.py,
each stage on the device's own inputs: the environment cube against the oracle's sky, the irradiance and specular cubes and the BRDF LUT
against the restatement fed the device's environment map, a known answer at roughness 0, the deferred pass, the sky and rt_reflections
with IBL, the reference's default view, the gates and isolation, the 1080p frame with IBL and the C++ mirror."""
import numpy as np
import pytest

import hybrid_reference as hr
import ibl_reference as ir
import rust_renderer_amd as rr
from hybrid_util import (assets, check_ibl_frame, cpp_scene, cpp_view, ibl_view, pair, read_all, record, run_cpp, scene_named,  # noqa: F401
                         synthetic_scene, ulps)
from rust_renderer_amd.api import UtopianError

pytestmark = pytest.mark.gpu

ENV = rr.HYBRID_ENVIRONMENT
# tolerances (DESIGN.md section 2 "Environment and IBL maps"): the environment is the sky pass's integrator (the sky pass's tolerance);
# the irradiance filter has no transcendental on the device (the tap table is made on the host) and matches to IRR_ULP; the specular
# filter's random() goes through device sinf and its lod through log2f (SPEC_RTOL); the LUT through sinf / cosf / powf, within one
# fp16 ulp after rounding; the consumers read the device's maps with the same arithmetic as the restatement (CONSUMER_ULP, hybrid_util)
IRR_ULP = 2
SPEC_RTOL = 2e-3


def eye_of(view):
    return np.array(view.inverse_view[12:15], np.float32)


def sample_texels(S, seed):
    """a fixed sample of one face's texels: the four corners, points on the four edges and random interior texels"""
    rng = np.random.default_rng(seed)
    e = [0, S - 1]
    ij = [(i, j) for i in e for j in e] + [(0, S // 2), (S - 1, S // 3), (S // 4, 0), (S // 2 + 1, S - 1)]
    ij += [tuple(x) for x in rng.integers(0, S, (6, 2))]
    a = np.array(ij)
    return a[:, 0], a[:, 1]


def interior_texels(S, seed):
    """eight texels strictly inside a face: the four around its centre and four random ones"""
    rng = np.random.default_rng(seed)
    c = S // 2
    a = np.array([(c - 1, c - 1), (c, c - 1), (c - 1, c), (c, c)] + [tuple(x) for x in rng.integers(1, S - 1, (4, 2))])
    return a[:, 0], a[:, 1]


# mips 5, 6 and 7 (16^2, 8^2, 4^2 per face) are compared at every texel: they hold the partial last block of k_env_cube's and
# k_env_specular's linear texel index (2,097,120 texels = 8,191.875 blocks of 256)
EVERY_TEXEL_MIPS = (5, 6, 7)


def texels_of(S, seed, m):
    if m in EVERY_TEXEL_MIPS:
        j, i = np.mgrid[0:S, 0:S]
        return i.reshape(-1), j.reshape(-1)
    return sample_texels(S, seed)


@pytest.fixture(scope="module")
def built():
    """one context with the maps built for the synthetic scene's view, and those maps read back"""
    scene = synthetic_scene()
    gpu, cpu, meshes = pair(scene)
    v = ibl_view(scene)
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | ENV)
    return dict(scene=scene, gpu=gpu, cpu=cpu, meshes=meshes, view=v, maps=ir.read_maps(gpu))


# ---- 1-4. the four maps ---------------------------------------------------------------------------------------------------------
def test_environment_texels_equal_the_sky_on_every_face_mip_edge_and_corner(built):
    v, env = built["view"], built["maps"]["env"]
    worst = 0.0
    for m in range(ir.MIPS):
        S = ir.SIZE >> m
        assert env[m].shape == (6, S, S, 4) and (env[m][..., 3] == 1.0).all() and np.isfinite(env[m]).all()
        for f in range(6):
            i, j = texels_of(S, 10 * m + f, m)
            want = ir.environment(eye_of(v), v.sun_dir[:], f, i, j, S)
            got = env[m][f, j, i, :3]
            worst = max(worst, float(np.max(np.abs(got - want) / (np.abs(want) + 1e-6))))
            assert np.allclose(got, want, rtol=1e-4, atol=1e-6), (m, f)
    record("ibl", "environment", max_rel=worst)
    s = built["gpu"].environment_stats()
    assert s.builds == 1 and all(ms > 0 for ms in s.pass_ms)
    assert np.array_equal(np.array(s.sun_dir[:], np.float32), np.array(v.sun_dir[:], np.float32)) and np.array_equal(np.array(s.eye[:], np.float32), eye_of(v))


def test_irradiance_equals_the_restatement_on_the_device_environment(built):
    maps = built["maps"]
    taps = ir.irradiance_taps()
    worst = 0
    for f in range(6):
        i, j = sample_texels(ir.SIZE, 100 + f)
        ii, jj = interior_texels(ir.SIZE, 100 + f)
        i, j = np.concatenate([i[:8], ii]), np.concatenate([j[:8], jj])  # corners and edges, and the interior
        want = ir.irradiance(maps["env"][0], f, i, j, taps)
        got = maps["irr"][f, j, i, :3]
        u = ulps(got, want)
        worst = max(worst, int(u.max()))
        assert u.max() <= IRR_ULP, (f, u.max())
    assert (maps["irr"][..., 3] == 1.0).all() and np.isfinite(maps["irr"]).all()
    record("ibl", "irradiance", max_ulp=worst)


def test_every_specular_mip_equals_the_restatement_on_the_device_environment(built):
    maps = built["maps"]
    worst, wrapped = 0.0, 0
    for m in range(ir.MIPS):
        S = ir.SIZE >> m
        for f in range(6):
            i, j = texels_of(S, 200 + 10 * m + f, m)
            want = ir.specular(maps["env"], m, f, i, j)
            got = maps["spec"][m][f, j, i, :3]
            ok = np.isclose(got, want, rtol=SPEC_RTOL, atol=1e-7).all(axis=1)
            if not ok.all():
                # random(N.xz) = fract(sin(.) * 43758.5453) jumps by ~1 where that product crosses an integer: there, one ulp of sinf
                # (device) against numpy's sin turns every tap's phi by ~0.1 rad. Such a texel may match the other branch instead,
                # and only if its random() does wrap within two ulps of the sine
                bad = ~ok
                r0 = ir.random2(*ir.texel_dir(f, i[bad], j[bad], S)[:, [0, 2]].T)
                alt = np.zeros(bad.sum(), bool)
                for k in (-2, -1, 1, 2):
                    wraps = np.abs(ir.random2(*ir.texel_dir(f, i[bad], j[bad], S)[:, [0, 2]].T, sin_ulps=k) - r0) > 0.5
                    other = ir.specular(maps["env"], m, f, i[bad], j[bad], sin_ulps=k)
                    alt |= wraps & np.isclose(got[bad], other, rtol=SPEC_RTOL, atol=1e-7).all(axis=1)
                wrapped += int(alt.sum())
                want[np.nonzero(bad)[0][alt]] = got[np.nonzero(bad)[0][alt]]
            rel = np.abs(got - want) / (np.abs(want) + 1e-7)
            worst = max(worst, float(rel.max()))
            assert np.allclose(got, want, rtol=SPEC_RTOL, atol=1e-7), (m, f, rel.max())
    record("ibl", "specular", max_rel=worst, texels_at_a_random_wrap=wrapped)


def test_the_whole_brdf_lut_after_fp16_rounding(built):
    lut = built["maps"]["lut"]
    assert lut.shape == (512, 512, 2) and lut.dtype == np.float16
    want = ir.brdf_lut().astype(np.float16)
    d = np.abs(lut.view(np.int16).astype(np.int32) - want.view(np.int16).astype(np.int32))
    record("ibl", "brdf_lut", max_fp16_ulp=int(d.max()), exact=float((d == 0).mean()))
    assert d.max() <= 1, d.max()


def test_specular_mip0_is_the_environment_mip0_mirrored_in_y(built):
    """known answer: at roughness 0 every tap is the texel's own direction, which reads environment texel (i, S - 1 - j) of layer f, with
    layers 2 and 3 swapped (the cube is mirrored in y). The filter sums 32 products of that texel and dotNL (which is 1 to an ulp) and
    divides by the sum of the dotNL: at most 31 roundings of half an ulp each, so 16 ulp"""
    env0, spec0 = built["maps"]["env"][0], built["maps"]["spec"][0]
    for f in range(6):
        mirrored = env0[[0, 1, 3, 2, 4, 5][f], ::-1]
        u = ulps(spec0[f, ..., :3], mirrored[..., :3])
        assert u.max() <= 16, (f, u.max())


# ---- 5. the consumers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic", "spheres"])
def test_deferred_sky_and_reflections_with_ibl_equal_the_restatement(assets, name):
    scene = scene_named(name, assets)
    gpu, cpu, meshes = pair(scene)
    v = ibl_view(scene)
    v.num_lights = 0
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | ENV)
    maps = ir.read_maps(gpu)
    check_ibl_frame(gpu, cpu, meshes, v, maps, name)
    # and without SSAO and the ray-traced inputs
    v2 = ibl_view(scene, ssao_enabled=0, raytracing_supported=0)
    v2.num_lights = 0
    check_ibl_frame(gpu, cpu, meshes, v2, maps, name + "-plain")


def test_the_reference_default_view_renders_a_present_image():
    """UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT with the prototype's flags (shadows_enabled cleared): one call, from a fresh context"""
    scene = synthetic_scene()
    gpu, cpu, meshes = pair(scene)
    v = ibl_view(scene)
    gpu.render_hybrid(v, rr.HYBRID_FRAME | ENV)
    p = gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    assert (p[..., 3] == 255).all() and p[..., :3].std() > 5
    s = gpu.hybrid_frame_stats()
    assert all(ms > 0 for ms in s.pass_ms) and gpu.environment_stats().builds == 1
    # the same image as building first and rendering after
    b, _, _ = pair(scene)
    b.render_hybrid(v, rr.HYBRID_GBUFFER | ENV)
    b.render_hybrid(v, rr.HYBRID_FRAME)
    b.render_hybrid(v, rr.HYBRID_FRAME)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    assert np.array_equal(gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT), b.read_hybrid(rr.HYBRID_PRESENT_OUTPUT))


# ---- gates and isolation ------------------------------------------------------------------------------------------------------------
def test_read_back_gates():
    scene = synthetic_scene()
    gpu, _, _ = pair(scene)
    with pytest.raises(UtopianError, match="INVALID_ARGUMENT"):
        gpu.read_environment(rr.ENV_ENVIRONMENT)
    assert gpu.environment_stats().builds == 0
    gpu.render_hybrid(ibl_view(scene), ENV)
    for which, face, mip in ((rr.ENV_ENVIRONMENT, 6, 0), (rr.ENV_ENVIRONMENT, -1, 0), (rr.ENV_IRRADIANCE, 0, 1), (rr.ENV_BRDF_LUT, 1, 0)):
        with pytest.raises(UtopianError, match="INVALID_ARGUMENT"):
            gpu._check(gpu._api.read_environment(gpu._ctx, which, face, mip, np.empty(512 * 512 * 4, np.float32).ctypes.data))
    with pytest.raises(ValueError):
        gpu.read_environment(rr.ENV_SPECULAR, 0, 8)


def test_a_build_changes_no_other_image_and_no_stats():
    scene = synthetic_scene()
    a, _, _ = pair(scene)
    b, _, _ = pair(scene)
    v = ibl_view(scene)
    v.ibl_enabled = v.cubemap_enabled = 0
    for r in (a, b):
        r.render_hybrid(v, rr.HYBRID_FRAME)
    b.render_hybrid(v, ENV)
    a.render_hybrid(v, rr.HYBRID_FRAME)
    b.render_hybrid(v, rr.HYBRID_FRAME | ENV)
    ia, ib = read_all(a), read_all(b)
    for i in range(9):
        assert np.array_equal(ia[i].view(np.uint8), ib[i].view(np.uint8)), i
    sa, sb = a.hybrid_stats(), b.hybrid_stats()
    assert list(sa.rays) == list(sb.rays) and sa.reflection_pixels == sb.reflection_pixels
    st_a, st_b = a.get_stats(), b.get_stats()
    assert list(st_a.rays) == list(st_b.rays) and st_a.frames == st_b.frames


def test_maps_persist_go_stale_with_the_sun_and_stay_per_context():
    scene = synthetic_scene()
    gpu, _, _ = pair(scene)
    other, _, _ = pair(scene)
    v = ibl_view(scene)
    gpu.render_hybrid(v, ENV)
    first = ir.read_maps(gpu)
    built_ms = list(gpu.environment_stats().pass_ms)
    moved = ibl_view(scene)
    moved.sun_dir[:] = tuple(np.float32(np.array([0.3, 0.5, -0.81]) / np.linalg.norm([0.3, 0.5, -0.81])))
    gpu.render_hybrid(moved, rr.HYBRID_FRAME)  # no bit: the maps stay as they were, as in the reference
    assert list(gpu.environment_stats().pass_ms) == built_ms, "the stats stay the last build's"
    stale = ir.read_maps(gpu)
    for k in ("irr", "lut"):
        assert np.array_equal(first[k].view(np.uint8), stale[k].view(np.uint8)), k
    assert all(np.array_equal(a, b) for a, b in zip(first["env"], stale["env"]))
    assert gpu.environment_stats().builds == 1
    with pytest.raises(UtopianError):
        other.read_environment(rr.ENV_ENVIRONMENT)  # a second context has none
    other.render_hybrid(moved, rr.HYBRID_GBUFFER | ENV)
    gpu.render_hybrid(moved, ENV)  # the next build takes the new sun
    new = ir.read_maps(gpu)
    assert not np.array_equal(first["env"][0], new["env"][0])
    for f in range(6):
        assert np.array_equal(new["env"][0][f], other.read_environment(rr.ENV_ENVIRONMENT, f, 0))
    s = gpu.environment_stats()
    assert s.builds == 2 and np.array_equal(np.array(s.sun_dir[:], np.float32), np.array(moved.sun_dir[:], np.float32))


# ---- 1080p and the measured times ---------------------------------------------------------------------------------------------------
def test_1080p_config1_frame_with_ibl():
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    Wf, Hf = 1920, 1080
    gpu = rr.Renderer(Wf, Hf)
    meshes = hr.upload_recorded(scene, gpu, defaults=False)
    v = ibl_view(scene, Wf, Hf)
    v.num_lights = 0
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | ENV)
    env = gpu.environment_stats()
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    s = gpu.hybrid_frame_stats()
    d = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    assert np.isfinite(d).all()
    record("ibl", "config1-1080p-ibl", frame_ms=round(sum(s.pass_ms), 4), **{f"ms{k}": round(s.pass_ms[k], 4) for k in range(7)},
           **{f"env{k}": round(env.pass_ms[k], 3) for k in range(4)})
    assert all(ms > 0 for ms in s.pass_ms)


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_reads_a_map_and_renders_an_ibl_frame(tmp_path):
    meshes, v = cpp_scene(), cpp_view()
    v.shadows_enabled = 0
    v.ibl_enabled = v.cubemap_enabled = 1
    res, blob_out, r = run_cpp(tmp_path, "ibl", meshes, v, timeout=300)
    r.render_hybrid(v, rr.HYBRID_FRAME | ENV)
    mine = np.concatenate([r.read_environment(rr.ENV_IRRADIANCE, 2, 0).view(np.uint8).reshape(-1), r.read_hybrid(rr.HYBRID_PRESENT_OUTPUT).reshape(-1)])
    assert np.array_equal(blob_out, mine)
    assert f"builds {r.environment_stats().builds}" in res.stdout

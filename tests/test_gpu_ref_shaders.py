"""GPU: the HIP kernels against the reference's own shader text, no oracle in the loop.

Expected values are the recordings of tests/golden/ref_shader_kat.npz (made from the reference's compiled GLSL include files by
tests/golden/make_ref_shader_kat.py) and, for the deferred pass, oracle/_ref/libref_shaders.so where it is present. The reference
checkout is never read. What joins the reference's functions into a pass - the order of calls in a raygen, the frame-number and
seed convention, the G-buffer fetch, the primary ray's matrix lines - is still this repository's reading, named in each test."""
import os

import numpy as np
import pytest

import hybrid_frame_reference as fr
import ref_shaders as rs
import rust_renderer_amd as rr
from hybrid_util import DEFERRED_ULP, frame_view, gbuf, pair, synthetic_scene
from test_ref_shaders import SKY_REL, check_initial_ris, check_sky, ulps

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
W, H = 16, 8
# deferred with its own per-light term against deferred with the compiled surfaceShading, on the synthetic scene's 16 x 12 G-buffer,
# shadows, reflections and SSAO as the oracle computes them (96 geometry pixels, the view of test_deferred_lighting), measured on the
# CPU for the four light sets below: 3, 2, 3 and 2 ulp (powf(x, 5) against ((x x)(x x)) x; v / sqrt against v * (1 / sqrt)). With
# raytracing_supported = 0 the metal floor's own lighting shows too and the distance is 44 ulp (the NDF's denominator at low roughness)
DEFERRED_TERM_ON_SCENE_ULP = 3


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(GOLDEN, "ref_shader_kat.npz")))


# ---- initial RIS ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2])
def test_initial_ris(kat, ci):
    """uh_read_reservoirs(0) after the reset and initial-RIS passes alone, on a 16 x 8 context whose positions were written with
    uh_write_gbuffer_position, with 1, 3 and 1024 of the fixture's lights: against initRNG(pixel, size, frame) -> resample ->
    updateReservoir -> target_function -> finalize_resampling of the reference's compiled text. Y and M exact; W_sum and W_X bit for
    bit, because tests/test_ref_shaders.py found target_function bit-exact (RESAMPLE_ULP = 0).

    Still our reading: the order of those calls (initial_ris.rgen:19-39), the frame number int(total_samples + time * 10000), the
    seed from pixel and launch size, and the position fetch as the mean of the 2 x 2 texels up-left; make_shading_fixture.py reads
    them the same way. A search of frame numbers 0..8191 on the CPU found that at this size frame 4120 makes one pixel draw exactly
    1.0 for a candidate index, which then equals the light count; the frame is among those run, and the expected value has p_hat = 0
    for that index ("Pinned choices"). Pixel (4, 3) fetches a position equal to light 0's: distance 0"""
    check_initial_ris(lambda: rr.Renderer(W, H, device=0), kat, ci)


# ---- sky --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_sky(kat, case):
    """an empty scene at 16 x 8, one sample, against IntegrateScattering of the compiled text on oracle_api.primary_ray's rays (the
    jitter from the compiled initRNG / randomFloat) with the miss shader's clamp min(c, 1). The sun below the horizon, a view into a
    low sun (the clamp is reached), and a view steeply down at the ground. num_bounces is 1, the primary ray alone: with 0 the
    raygen's loop traces nothing and the frame is black, which is asserted too. The ray's matrix lines and the clamp are our reading
    of reference.rgen and reference.rmiss. Margin: the CPU bound SKY_REL, not below the 1e-4 the parity tests use"""
    check_sky(lambda: rr.Renderer(W, H, device=0), kat, case, max(SKY_REL, 1e-4))


# ---- deferred lighting ------------------------------------------------------------------------------------------------------------
DW, DH = 16, 12


def deferred_lights():
    """one light of each type above the synthetic scene"""
    out = []
    for t, pos, col, direction, spot in ((0.0, (0.0, 0.0, 0.0), (0.9, 0.7, 0.5), (0.3, -0.8, 0.4), 0.0),
                                         (1.0, (-1.0, 2.5, 2.0), (1.0, 0.6, 0.3), (0.0, -1.0, 0.0), 0.0),
                                         (2.0, (1.5, 3.0, 1.0), (0.4, 0.8, 1.0), (-0.2, -1.0, -0.3), 4.0)):
        l = rr.make_light(pos, color=col)
        l.light_type, l.spot = t, spot
        l.direction[:] = direction
        l.attenuation[:] = (0.8, 0.1, 0.2)
        out.append(l)
    return out


LIGHT_SETS = ((0,), (1,), (2,), (0, 1, 2))


def reference_term(P, base, N, metallic, roughness, light, eye):
    n = len(P)
    pixel = np.concatenate([P, base, N, metallic[:, None], roughness[:, None]], axis=1).astype(F)
    return rs.surface_shading(pixel, np.tile(light, (n, 1)), np.tile(eye, (n, 1)), np.ones(n, F))


@pytest.mark.parametrize("which", range(len(LIGHT_SETS)))
def test_deferred_lighting(which):
    """HYBRID_DEFERRED_OUTPUT on the geometry pixels of the synthetic scene at 16 x 12, one light of each type alone and all three
    together, against hybrid_frame_reference.deferred on the device's own G-buffer with surface_shading= the compiled surfaceShading
    (oracle/_ref/libref_shaders.so). Where that library is absent the term is deferred's own, which tests/test_ref_shaders.py holds
    to the recorded surfaceShading within SHADING_TERM_ULP. Bound: DEFERRED_ULP plus DEFERRED_TERM_ON_SCENE_ULP, the distance
    between deferred with either term measured on the CPU on this scene's G-buffer with these lights"""
    scene = synthetic_scene()
    gpu, _, meshes = pair(scene, DW, DH)
    lights = [deferred_lights()[i] for i in LIGHT_SETS[which]]
    for l in lights:
        gpu.add_gpu_light(l)
    gpu.initialize_raytracing()
    view = frame_view(scene, DW, DH, num_lights=len(lights))
    gpu.render_hybrid(view, rr.HYBRID_GBUFFER)  # rt_shadows reads the previous call's G-buffer: a steady frame
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    g, d = gbuf(gpu), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    images = (gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE))
    term = reference_term if rs.available() else None
    ref = fr.deferred(g, *images, view, meshes, lights, surface_shading=term)
    geo = g["position"][..., 3] == 1.0
    assert geo.sum() >= 40 and not geo.all() and np.isfinite(d[geo]).all()
    u = int(ulps(d[geo][:, :3], ref[geo][:, :3]).max())
    between = int(ulps(fr.deferred(g, *images, view, meshes, lights)[geo], ref[geo]).max()) if term else None
    print(f"deferred, lights {LIGHT_SETS[which]}: {u} ulp to the {'compiled' if term else 'own'} term; own to compiled term on this G-buffer: {between} ulp")
    assert u <= DEFERRED_ULP + DEFERRED_TERM_ON_SCENE_ULP, u

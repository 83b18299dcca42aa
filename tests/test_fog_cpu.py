"""CPU: the numpy restatement of the volumetric fog pass (tests/fog_reference.py) held to answers nobody computed with it, on the oracle's
own G-buffer: a bare floor against the closed form 1 - exp(-density D), the slab scene's shafts against a float64 geometric predicate
(with the adequacy of that scene for the GPU test's camera, size and step counts), density 0, and the phase function's normalisation.
test_gpu_fog.py holds the device to the restatement and runs the same known answers there."""
import numpy as np
import pytest

import fog_reference as fog
import hybrid_reference as hr
import oracle_api as oa
from hybrid_util import frame_view

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

W, H = fog.W, fog.H
F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32: one rounding is within U relative, one ulp is at most 2 U relative


def world(scene, view):
    """the scene on the oracle and the oracle's G-buffer of it"""
    cpu = oa.OracleRenderer(W, H)
    meshes = hr.upload_recorded(scene, cpu, True)
    return cpu, hr.gbuffer(cpu, meshes, view, W, H)


# ---- (a) a bare floor ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 7, 16, 32])
def test_a_bare_floor_is_lit_everywhere_and_F_is_the_closed_form(steps):
    """Every mask is (1 << steps) - 1, and F = (1 - a) * sum_k a^k telescopes to 1 - a^steps = 1 - exp(-density D). The bound, per pixel,
    relative to that: x = density * dt carries two roundings, so the exact exp of the float x is within 2 U x of exp(-density D / steps),
    and a is within two ulp (4 U) of that: e_a = 4 U + 2 U x. p_k = a^k carries k such errors and k roundings; the sum carries `steps`
    roundings; 1 - a carries the error of a, a e_a / (1 - a) relative, and one rounding; the final product one more; then the second
    order."""
    scene = fog.floor_scene()
    view = frame_view(scene, W, H)
    cpu, g = world(scene, view)
    p = fog.default_params(steps=steps, density=0.05, blur_radius=0)
    mask, (pixels, rays, lit) = fog.masks(cpu, g["position"], view, steps, p["max_distance"])
    _, _, D, marched = fog.rays(g["position"], view, p["max_distance"])
    geo = g["position"][..., 3].reshape(-1) != 0
    assert marched.all() and geo.any() and not geo.all() and pixels == W * H
    assert (mask == (1 << steps) - 1).all() and lit == rays == steps * W * H
    if steps == 32:
        assert (mask >> 31).all()
    a, Ttot, Fr = fog.resolve(mask, D, marched, steps, p["density"])
    D64 = D.astype(np.float64)
    x = 0.05 * D64 / steps
    exact_a = np.exp(-x)
    want = 1.0 - np.exp(-0.05 * D64)
    e_a = 4 * U + 2 * U * x
    first = exact_a * e_a / (1.0 - exact_a) + U + steps * (e_a + U) + steps * U + U
    bound = (first + (steps * (e_a + 2 * U)) ** 2 + first ** 2) * want
    err = np.abs(Fr.astype(np.float64) - want)
    print(f"steps {steps}: D {D.min():.2f}..{D.max():.2f}, F {Fr.min():.4f}..{Fr.max():.4f}, max error {err.max():.3e}, largest error / bound {(err / bound).max():.3f}")
    assert (D[~geo] == F(200.0)).all() and (err <= bound).all()
    # and Ttot is a^steps
    assert np.abs(Ttot.astype(np.float64) - np.exp(-0.05 * D64)).max() <= (steps * (e_a.max() + U) * 1.001)


# ---- (b) the slab with a hole ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab():
    scene = fog.slab_scene()
    view = fog.slab_view(scene)
    return (view,) + world(scene, view)


@pytest.mark.parametrize("steps", [1, 7, 32])
def test_the_slab_scenes_shafts_equal_the_float64_predicate(slab, steps):
    """the camera, size and step counts of test_gpu_fog.py: at most 2 % of the samples lie within 1e-3 of a shadow boundary or of the
    sheet and are left out; of the rest at least a tenth is lit and a tenth dark, and each agrees with the predicate"""
    view, cpu, g = slab
    mask, (pixels, rays, lit_total) = fog.masks(cpu, g["position"], view, steps, fog.SLAB_MAX_DISTANCE)
    rows, X = fog.sample_points(g["position"], view, steps, fog.SLAB_MAX_DISTANCE)
    lit, compared, inside = fog.slab_predicate(X, hr.sun_direction(view))
    got = ((mask.reshape(-1)[rows][:, None] >> np.arange(steps, dtype=np.uint32)[None, :]) & 1).astype(bool)
    left_out = 1.0 - compared.mean()
    frac_lit, frac_dark = lit[compared].mean(), (~lit[compared]).mean()
    print(f"steps {steps}: {rays} samples, {left_out:.4%} left out, {frac_lit:.3f} lit, {frac_dark:.3f} dark, {(got != lit)[compared].sum()} disagree")
    assert pixels == W * H and rays == pixels * steps and inside.all(), "every sample below the sheet projects well inside its span"
    assert left_out <= 0.02
    assert frac_lit >= 0.10 and frac_dark >= 0.10
    assert np.array_equal(got[compared], lit[compared])
    assert lit_total == got.sum()


# ---- (c) density 0 ----------------------------------------------------------------------------------------------------------------
def test_density_0_leaves_every_finite_colour_bit_identical(slab):
    """a = exp(-0) = 1: Ttot = 1 and F = (1 - 1) * sum = 0, so out = (C * 1 + S * 0) + ambient * 0 = C. (The one exception IEEE addition
    makes is a channel that is -0.0, which comes out +0.0; deferred_output holds none.)"""
    view, cpu, g = slab
    rng = np.random.default_rng(11)
    C = (rng.standard_normal((H, W, 4)) * np.float32(10.0) ** rng.integers(-20, 20, (H, W, 4))).astype(np.float32)
    C[0, 0, :3], C[0, 1, :3] = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    for r in (0, 2):
        p = fog.default_params(steps=7, density=0.0, blur_radius=r, max_distance=fog.SLAB_MAX_DISTANCE, intensity=3.0)
        mask, _ = fog.masks(cpu, g["position"], view, 7, fog.SLAB_MAX_DISTANCE)
        terms, out = fog.shade(mask, g["position"], C, view, p)
        assert mask.any() and (terms[..., 0] == 1).all() and (terms[..., 1] == 1).all() and not terms[..., 2:].any()
        assert np.array_equal(out.view(np.uint32), C.view(np.uint32))
    # and with a density the frame does change
    terms, out = fog.shade(mask, g["position"], C, view, fog.default_params(steps=7, density=0.1, max_distance=fog.SLAB_MAX_DISTANCE))
    assert (out[..., :3] != C[..., :3]).any() and np.array_equal(out[..., 3].view(np.uint32), C[..., 3].view(np.uint32))


# ---- (d) the phase function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [-0.9, 0.0, 0.6, 0.95])
def test_the_phase_function_integrates_to_one(g):
    """2 pi int_{-1}^{1} ph(c) dc = 1 by Gauss-Legendre quadrature in float64 over the float32 values. Their pointwise relative error: c
    rounded to float32 and the three roundings of q are within 5 U (1 + g g) of q in absolute terms, q >= (1 - |g|)^2, q sqrt(q)
    multiplies that by 1.5, and the remaining products and the quotient add 6 U; a positive integrand with that pointwise error
    integrates to within it. The quadrature itself is held to 1e-9 on the closed form."""
    nodes, weights = np.polynomial.legendre.leggauss(4000)
    direction = np.stack([np.zeros_like(nodes), np.zeros_like(nodes), nodes], axis=-1).astype(np.float32)
    ph = fog.phase(np.float32([0.0, 0.0, 1.0]), direction, g).astype(np.float64)
    closed = (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * nodes) ** 1.5)
    eps = 1.5 * 5 * U * (1 + g * g) / (1 - abs(g)) ** 2 + 6 * U + abs(float(fog.PI) - np.pi) / np.pi
    total, exact = 2 * np.pi * (weights * ph).sum(), 2 * np.pi * (weights * closed).sum()
    print(f"g {g}: integral {total:.9f} (closed form by the same quadrature {exact:.12f}), bound {eps:.3e}, max pointwise {np.abs(ph / closed - 1).max():.3e}")
    assert abs(exact - 1) <= 1e-9 and (ph > 0).all()
    assert abs(total - 1) <= eps + 1e-9 and np.abs(ph / closed - 1).max() <= eps
    if g > 0:
        assert ph[-1] > ph[0], "forward scattering: brightest toward the sun"


def test_the_filter_and_the_march_rules():
    """the filter on a hand-made frame: radius 0 is the identity, a depth step stops it, a pixel that did not march is no tap and gets
    0; a geometry pixel with a non-finite or zero-length V does not march and keeps its colour"""
    Hh, Ww = 5, 9
    D = np.full((Hh, Ww), 10.0, np.float32)
    D[:, 5:] = 20.0
    marched = np.ones((Hh, Ww), bool)
    marched[2, 2] = False
    Fr = np.arange(Hh * Ww, dtype=np.float32).reshape(Hh, Ww) / F(64.0)
    Fr[~marched] = 0
    flat = lambda a: a.reshape(-1)
    assert np.array_equal(fog.blur(flat(Fr), flat(D), flat(marched), Ww, Hh, 0, 0.1), flat(Fr))
    out = fog.blur(flat(Fr), flat(D), flat(marched), Ww, Hh, 1, 0.1).reshape(Hh, Ww)
    assert out[2, 2] == 0
    taps = [Fr[yy, xx] for yy in (1, 2, 3) for xx in (3, 4)]  # (2, 4): the column x = 5 lies 10 away, beyond 0.1 * 10
    total = F(0.0)
    for t in taps:
        total = total + t
    assert out[2, 4] == total / F(6.0)
    taps = [Fr[yy, xx] for yy in (0, 1) for xx in (0, 1)]  # the corner: four taps in the frame
    assert out[0, 0] == (((taps[0] + taps[1]) + taps[2]) + taps[3]) / F(4.0)
    taps = [Fr[yy, xx] for yy in (0, 1, 2) for xx in (1, 2, 3) if marched[yy, xx]]  # next to the pixel that did not march
    total = F(0.0)
    for t in taps:
        total = total + t
    assert out[1, 2] == total / F(8.0)
    # the march rule
    scene = fog.floor_scene()
    view = frame_view(scene, W, H)
    pos = np.zeros((1, 4, 4), np.float32)
    o = np.float32(view.inverse_view[12:15])
    pos[0, 0] = (np.nan, 0, 0, 1)
    pos[0, 1] = (np.inf, 0, 0, 1)
    pos[0, 2] = (*o, 1)
    pos[0, 3] = (0, 0, 0, 1)
    _, _, Dm, m = fog.rays(pos, view, 200.0)
    assert m.tolist() == [False, False, False, True] and (Dm[:3] == 0).all() and Dm[3] > 0

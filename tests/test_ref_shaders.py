"""CPU: the oracle and the numpy second readings against the reference's OWN shader text.

tests/golden/ref_shader_kat.npz holds results recorded from the reference's random.glsl, restir_sampling.glsl, brdf.glsl,
atmosphere.glsl and pbr_lighting.glsl's surfaceShading as oracle/ref_shaders compiles them (tests/golden/make_ref_shader_kat.py).
Every other known-answer file of this suite is a reading of that text by this repository's authors; a line misread the same way
by the oracle, its numpy restatement and the kernel passed them all. These tests compare with recorded data, so they run where
neither the reference checkout nor oracle/_ref exists; only test_fixture_regenerates needs one of the two.

Tolerances. Integers, RNG states and float results of functions that use only + - * /, sqrt, comparisons and conversions: bit for
bit (NaN equals NaN). Functions through pow, exp, sin, cos or a normalize that is evaluated differently (the compiled text divides
by sqrt(dot); the oracle and the restatements multiply by 1 / sqrt(dot)) get twice the largest distance measured on this
fixture against the x86-64 glibc build of the oracle and numpy 2.2; each constant below has its measurement beside it."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_api as oa
import ref_shaders as rs
import rust_renderer_amd as rr
from rust_renderer_amd.types import VERTEX_DTYPE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32

# ---- the measured margins (measured -> bound = 2 x measured) -------------------------------------------------------------------
TARGET_FUNCTION_ULP = 0       # measured 0: powf(d, 2) of the compiled text equals the oracle's and the restatement's d * d on every vector
RESAMPLE_ULP = 0              # measured 0 (follows from the line above: the rest is + * / and comparisons)
PBR_WEIGHT_ULP = 98           # measured 49 (roughness 0.3 .. 1): powf(x, 5) against ((x x)(x x)) x, the two normalizes, and the NDF's denominator
                              # N.H^2 (a^2 - 1) + 1, which cancels to a^2 near N.H = 1 and multiplies one ulp of H by 1 / a^2
SKY_REL = 2.2e-5              # measured 1.07e-5 through oa.sky (it normalises the sun once more); IntegrateScattering and
                              # IntegrateOpticalDepth called directly measured 0. Below the 3e-5 of test_oracle_kat.py
NUMPY_SKY_REL = 6.5e-7        # measured 3.24e-7: numpy's float32 exp and power against libm's
IBL_RANDOM_ABS = 0.0078125    # measured 0.00390625: one float32 ulp of numpy's sine, times 43758.5453
IBL_GGX_ULP = 32              # measured 16: numpy's float32 sin / cos and the two normalizes
SHADING_TERM_ULP = 240        # measured 120, deferred and forward alike (as PBR_WEIGHT_ULP, over all roughnesses of the fixture)


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(GOLDEN, "ref_shader_kat.npz")))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def msf():
    return _load("make_shading_fixture")


def same_bits(a, b):
    """bit for bit, NaN equal to NaN (any payload)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulps(a, b):
    """float32 ulp distance; NaN to NaN is 0, NaN to a number and infinities of different sign are 2^32"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    ka, kb = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ka, kb = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka), np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    d = np.abs(ka - kb)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.where(na & nb, 0, np.where(na | nb, 1 << 32, d))
    return np.where(np.isinf(a) & np.isinf(b) & (a != b), 1 << 32, d)


def rel(got, want, floor=1e-9):
    """largest |got - want| per vector over the vector's largest |want| (rows); non-finite components must agree exactly"""
    got, want = np.asarray(got, np.float64).reshape(len(got), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    fin = np.isfinite(want)
    assert (np.isnan(got) == np.isnan(want)).all() and (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()
    scale = np.maximum(np.max(np.where(fin, np.abs(want), 0.0), axis=1), floor)
    return float(np.max(np.where(fin, np.abs(got - want), 0.0) / scale[:, None]))


def within(name, measured, bound):
    print(f"{name}: measured {measured!r}, bound {bound!r}")
    assert measured <= bound, f"{name}: {measured!r} > {bound!r}"


def reservoirs_equal(got, want):
    """Y and M exact -> the largest ulp distance of W_sum and W_X"""
    assert np.array_equal(got["Y"], want["Y"]) and np.array_equal(got["M"], want["M"])
    return int(max(ulps(got["W_sum"], want["W_sum"]).max(), ulps(got["W_X"], want["W_X"]).max()))


def light_struct(row):
    return rr.types.GpuLight.from_buffer_copy(np.ascontiguousarray(row, F).tobytes())


def oracle_with_lights(rows):
    o = oa.OracleRenderer(4, 4)
    for row in rows:
        o.add_gpu_light(light_struct(row))
    return o


# ---- the fixture itself ------------------------------------------------------------------------------------------------------
def test_fixture_regenerates(tmp_path):
    """the committed file is what the reference's text gives today: regenerated from oracle/_ref/libref_shaders.so (built from the
    checkout where there is one) and compared byte for byte. Skips only where there is neither library nor checkout"""
    if not rs.available():
        pytest.skip("neither oracle/_ref/libref_shaders.so nor the reference checkout is here")
    gen = _load("make_ref_shader_kat")
    path = str(tmp_path / "ref_shader_kat.npz")
    gen.write(path, gen.generate())
    assert open(path, "rb").read() == open(os.path.join(GOLDEN, "ref_shader_kat.npz"), "rb").read()


def test_fixture_is_small_and_mostly_finite(kat):
    assert os.path.getsize(os.path.join(GOLDEN, "ref_shader_kat.npz")) < 200 * 1024
    for key in ("tf_out", "ggx_out", "is_out", "ss_out", "sky_color", "sky_transmittance", "od_out", "si_out", "pm_out", "gs_out", "gsm_out"):
        a = kat[key].reshape(len(kat[key]), -1)
        assert (~np.isfinite(a).all(axis=1)).mean() <= 0.10, key
    assert (kat["rf_value"][:6] == 1.0).all() and (kat["rf_value"] <= 1.0).all()


def test_brdf_pieces_agree_with_float64(kat):
    """DistributionGGX, GeometrySchlickGGX, GeometrySmith, fresnelSchlick and fresnelSchlickRoughness as recorded one by one, against
    the formulas of learnopengl.com/PBR (which brdf.glsl cites) in float64 on the finite vectors: the translation kept them float32
    functions of the stated shape (a literal left double, or an operand order changed, would not show as bits here - the
    comparisons below with code of ours hold the bits). 2e-5 relative: 24-bit arithmetic through a^4 and a quotient"""
    f = lambda key: kat[key].astype(np.float64)
    dot = lambda a, b: (a * b).sum(axis=1)
    a2 = f("ggx_rough") ** 4
    ndh = np.maximum(dot(f("ggx_N"), f("ggx_H")), 0.0)
    PI = np.float64(F(3.14159265359))
    with np.errstate(all="ignore"):
        ggx = a2 / (PI * (ndh * ndh * (a2 - 1.0) + 1.0) ** 2)
    ok = np.isfinite(kat["ggx_out"]) & (kat["ggx_rough"] > 0.05)
    assert ok.mean() > 0.8 and np.allclose(kat["ggx_out"][ok], ggx[ok], rtol=2e-4, atol=0)  # the denominator cancels: 1 / a^2 amplification
    g1 = lambda x, r: x / (x * (1.0 - (r + 1.0) ** 2 / 8.0) + (r + 1.0) ** 2 / 8.0)
    assert np.allclose(kat["gs_out"], g1(f("gs_ndv"), f("gs_rough")), rtol=2e-5, atol=0)
    ndv, ndl = np.maximum(dot(f("gsm_N"), f("gsm_V")), 0.0), np.maximum(dot(f("gsm_N"), f("gsm_L")), 0.0)
    assert np.allclose(kat["gsm_out"], g1(ndv, f("gsm_rough")) * g1(ndl, f("gsm_rough")), rtol=2e-5, atol=1e-9)
    x5 = np.clip(1.0 - f("fs_cos"), 0.0, 1.0)[:, None] ** 5
    assert np.allclose(kat["fs_out"], f("fs_F0") + (1.0 - f("fs_F0")) * x5, rtol=2e-5, atol=1e-7)
    hi = np.maximum(1.0 - f("fs_rough")[:, None], f("fs_F0"))
    assert np.allclose(kat["fsr_out"], f("fs_F0") + (hi - f("fs_F0")) * x5, rtol=2e-5, atol=1e-7)


# ---- the oracle: random.glsl ---------------------------------------------------------------------------------------------------
def test_oracle_rng_bit_for_bit(kat):
    assert [oa.jenkins_hash(int(x)) for x in kat["jenkins_in"]] == [int(x) for x in kat["jenkins_out"]]
    for (px, py, rx, _, fr), want in zip(kat["initrng_in"], kat["initrng_out"]):
        assert oa.init_rng(int(px), int(py), int(rx), int(fr)) == int(want)
    for s, v, s2 in zip(kat["rf_state_in"], kat["rf_value"], kat["rf_state_out"]):
        got, after = oa.random_floats(int(s), 1)
        assert after == int(s2) and same_bits(got, [v]).all()
    for s, p, s2 in zip(kat["sphere_state_in"], kat["sphere_out"], kat["sphere_state_out"]):
        got, after = oa.random_point_in_unit_sphere(int(s))
        assert after == int(s2) and same_bits(got, p).all()
    for s, p, s2 in zip(kat["disk_state_in"], kat["disk_out"], kat["disk_state_out"]):
        got, after = oa.random_point_in_unit_disk(int(s))
        assert after == int(s2) and same_bits(got, p).all()


# ---- the oracle: restir_sampling.glsl -------------------------------------------------------------------------------------------
def test_oracle_target_function(kat):
    """index 1024 is one past the 1024 lights the oracle is given: the reference's text reads the filled slot, the oracle answers 0
    ("Pinned choices": light index out of range has p_hat = 0). The test asserts that and compares the rest"""
    o = oracle_with_lights(kat["lights"][:1024])
    got = np.array([o.target_function(int(i), p) for i, p in zip(kat["tf_index"], kat["tf_pos"])], F)
    past = kat["tf_index"] >= 1024
    assert past.any() and (got[past] == 0.0).all() and (kat["tf_out"][past] != 0.0).all()
    within("target_function ulp", int(ulps(got[~past], kat["tf_out"][~past]).max()), TARGET_FUNCTION_ULP)
    d = oracle_with_lights(kat["lights_dark"][:2])
    got = np.array([d.target_function(int(i), p) for i, p in zip(kat["tf_dark_index"], kat["tf_dark_pos"])], F)
    assert same_bits(got, kat["tf_dark_out"]).all() and np.isnan(got[0]) and (got[1:] == 0).all()


def test_oracle_sample_light_uniform_bit_for_bit(kat):
    for c, (nl, mx) in enumerate(kat["ris_configs"]):
        for j, s in enumerate(kat["slu_state_in"]):
            i, w, after = oa.sample_light_uniform(int(nl), int(mx), int(s))
            assert (i, after) == (int(kat["slu_index"][c, j]), int(kat["slu_state_out"][c, j])) and same_bits([w], [kat["slu_weight"][c, j]]).all()
        assert (kat["slu_index"][c, :6] == min(nl, mx)).all(), "a draw of exactly 1.0: the index equals the light count"


def test_oracle_update_and_finalize_bit_for_bit(kat):
    for j in range(len(kat["ur_state_in"])):
        r, after = oa.update_reservoir(int(kat["ur_state_in"][j]), kat["ur_res_in"][j], kat["ur_Xi"][j], kat["ur_w"][j], kat["ur_M"][j])
        w = kat["ur_res_out"][j]
        assert after == int(kat["ur_state_out"][j]) and (r["Y"], r["M"]) == (w["Y"], w["M"])
        assert same_bits([r["W_sum"], r["W_X"]], [w["W_sum"], w["W_X"]]).all()
    for j in range(len(kat["fz_p_hat"])):
        r, w = oa.finalize_resampling(kat["fz_res_in"][j], kat["fz_p_hat"][j]), kat["fz_res_out"][j]
        assert (r["Y"], r["M"]) == (w["Y"], w["M"]) and same_bits([r["W_sum"], r["W_X"]], [w["W_sum"], w["W_X"]]).all(), j


def _oracle_resample(o, nl, mx, states, pos):
    out = np.zeros(len(states), oa.RESERVOIR_DTYPE)
    after = np.zeros(len(states), np.uint32)
    for j, (s, p) in enumerate(zip(states, pos)):
        out[j], after[j] = o.resample(int(nl), int(mx), int(s), p)
    return out, after


def test_oracle_resample(kat):
    """Y, M and the RNG state exact, the weights within RESAMPLE_ULP. The first six states draw exactly 1.0 first, so the candidate
    index equals the light count: where that is one past the oracle's lights it answers p_hat = 0 ("Pinned
    choices"), which is what the reference's text gives with a dark light in that slot (rs_one_res); with 1024 lights of which 16
    are used, index 16 is a light like any other and the plain recording holds"""
    worst = 0
    for c, (nl, mx) in enumerate(kat["ris_configs"]):
        o = oracle_with_lights(kat["lights"][: min(int(nl), 1024)])
        got, after = _oracle_resample(o, nl, mx, kat["rs_state_in"], kat["rs_pos"])
        want, want_after = kat["rs_res"][c].copy(), kat["rs_state_out"][c].copy()
        if min(nl, mx) >= nl:
            want[:6], want_after[:6] = kat["rs_one_res"][c], kat["rs_one_state_out"][c]
        assert np.array_equal(after, want_after)
        worst = max(worst, reservoirs_equal(got, want))
    o = oracle_with_lights(kat["lights_dark"][:2])
    got, after = _oracle_resample(o, 2, 1024, kat["rs_state_in"], kat["rs_pos"])
    assert np.array_equal(after, kat["rs_dark_state_out"]) and (got["Y"] == -1).all()
    worst = max(worst, reservoirs_equal(got, kat["rs_dark_res"]))
    within("resample ulp", worst, RESAMPLE_ULP)


# ---- the oracle: brdf.glsl / surfaceShading through material type 4 ----------------------------------------------------------------
def test_oracle_cook_torrance_weight(kat):
    """material type 4 returns kD * baseColor + specular * pi for the scatter direction L (oracle.cpp's pbr_weight, what
    closest_hit_shader calls): surfaceShading of a white directional light along L, times pi / N.L. DistributionGGX,
    GeometrySchlickGGX, GeometrySmith and fresnelSchlick are all inside it"""
    px, PI = kat["pw_pixel"], F(3.14159265359)
    N, V, L = px[:, 6:9], kat["pw_V"], kat["pw_L"]
    got = np.array([oa.pbr_weight(N[j], V[j], L[j], px[j, 3:6], px[j, 9], px[j, 10]) for j in range(len(px))], F)
    ndl = (N[:, 0] * L[:, 0] + N[:, 1] * L[:, 1]) + N[:, 2] * L[:, 2]
    want = (kat["pw_out"] * PI) / ndl[:, None]
    assert (ndl > 0.2).all()
    within("pbr_weight ulp", int(ulps(got, want).max()), PBR_WEIGHT_ULP)


# ---- the oracle: atmosphere.glsl ----------------------------------------------------------------------------------------------------
def test_oracle_sphere_intersection_and_phase_mie_bit_for_bit(kat):
    got = np.array([oa.sphere_intersection(s, d, c, r) for s, d, c, r in zip(kat["si_start"], kat["si_dir"], kat["si_center"], kat["si_radius"])], F)
    assert same_bits(got, kat["si_out"]).all()
    assert (kat["si_out"][:, 0] == -1).any() and (kat["si_out"][:, 0] > 0).any()  # misses and starts outside are there
    got = np.array([oa.phase_mie(c, g) for c, g in zip(kat["pm_costh"], kat["pm_g"])], F)
    assert same_bits(got, kat["pm_out"]).all()


def test_oracle_sky(kat):
    n = len(kat["sky_origin"])
    od = np.array([oa.integrate_optical_depth(kat["sky_origin"][j], kat["sky_dir"][j]) for j in range(n)], F)
    within("IntegrateOpticalDepth rel", rel(od, kat["od_out"]), SKY_REL)
    res = [oa.integrate_scattering(kat["sky_origin"][j], kat["sky_dir"][j], kat["sky_length"][j], kat["sky_light_dir"][j], kat["sky_light_color"][j]) for j in range(n)]
    color, tr = np.array([r[0] for r in res], F), np.array([r[1] for r in res], F)
    within("IntegrateScattering rel", max(rel(color, kat["sky_color"]), rel(tr, kat["sky_transmittance"])), SKY_REL)
    # oa.sky is the entry point the parity tests use (it normalises the sun once more)
    n_hard = int(kat["sky_counts"][1])
    sky = np.array([oa.sky(kat["sky_origin"][j], kat["sky_dir"][j], kat["sky_light_dir"][j]) for j in range(n_hard)], F)
    within("oa.sky rel", rel(sky, kat["sky_color"][:n_hard]), SKY_REL)


# ---- the numpy second readings: make_shading_fixture.py ----------------------------------------------------------------------------
def test_numpy_rng_reading_bit_for_bit(kat, msf):
    assert [int(msf.jenkins_hash(x)) for x in kat["jenkins_in"]] == [int(x) for x in kat["jenkins_out"]]
    for (px, py, rx, _, fr), want in zip(kat["initrng_in"], kat["initrng_out"]):
        assert int(msf.init_rng(int(px), int(py), int(rx), fr)) == int(want)
    for s, v, s2 in zip(kat["rf_state_in"], kat["rf_value"], kat["rf_state_out"]):
        g = msf.Rng(s)
        assert same_bits([g.random_float()], [v]).all() and int(g.s) == int(s2)
    for s, p, s2 in zip(kat["sphere_state_in"], kat["sphere_out"], kat["sphere_state_out"]):
        g = msf.Rng(s)
        assert same_bits(g.point_in_unit_sphere(), p).all() and int(g.s) == int(s2)


def _msf_lights(msf, rows, nl, mx):
    return msf.Lights(rows[:, 4:7], rows[:, 16:19], nl, mx)


def test_numpy_ris_reading(kat, msf):
    lights = _msf_lights(msf, kat["lights"][:1024], 1024, 1024)
    got = np.array([lights.target_function(int(i), p) for i, p in zip(kat["tf_index"], kat["tf_pos"])], F)
    past = kat["tf_index"] >= 1024
    assert (got[past] == 0.0).all()  # DESIGN.md section 2, "Pinned choices"
    within("numpy target_function ulp", int(ulps(got[~past], kat["tf_out"][~past]).max()), TARGET_FUNCTION_ULP)
    for c, (nl, mx) in enumerate(kat["ris_configs"]):
        L = _msf_lights(msf, kat["lights"][:1024], int(nl), int(mx))
        for j, s in enumerate(kat["slu_state_in"]):
            g = msf.Rng(s)
            i, w = L.sample_uniform(g)
            assert (i, int(g.s)) == (int(kat["slu_index"][c, j]), int(kat["slu_state_out"][c, j])) and same_bits([w], [kat["slu_weight"][c, j]]).all()
    for j in range(len(kat["ur_state_in"])):
        g, r0, w = msf.Rng(kat["ur_state_in"][j]), kat["ur_res_in"][j], kat["ur_res_out"][j]
        r = {"Y": int(r0["Y"]), "W_sum": r0["W_sum"], "W_X": r0["W_X"], "M": int(r0["M"])}
        msf.update_reservoir(g, r, kat["ur_Xi"][j], kat["ur_w"][j], int(kat["ur_M"][j]))
        assert (r["Y"], r["M"], int(g.s)) == (w["Y"], w["M"], int(kat["ur_state_out"][j])) and same_bits([r["W_sum"]], [w["W_sum"]]).all()
    for j in range(len(kat["fz_p_hat"])):
        r0, w = kat["fz_res_in"][j], kat["fz_res_out"][j]
        r = {"Y": int(r0["Y"]), "W_sum": r0["W_sum"], "W_X": r0["W_X"], "M": int(r0["M"])}
        msf.finalize_resampling(r, kat["fz_p_hat"][j])
        assert same_bits([r["W_X"]], [w["W_X"]]).all(), j


def test_numpy_resample_reading(kat, msf):
    worst = 0
    for c, (nl, mx) in enumerate(kat["ris_configs"]):
        L = _msf_lights(msf, kat["lights"][: min(int(nl), 1024)], int(nl), int(mx))
        want, want_after = kat["rs_res"][c].copy(), kat["rs_state_out"][c].copy()
        if min(nl, mx) >= nl:
            want[:6], want_after[:6] = kat["rs_one_res"][c], kat["rs_one_state_out"][c]
        got = np.zeros(len(want), oa.RESERVOIR_DTYPE)
        for j, (s, p) in enumerate(zip(kat["rs_state_in"], kat["rs_pos"])):
            g = msf.Rng(s)
            r = msf.resample(L, g, p)
            got[j] = (r["Y"], r["W_sum"], r["W_X"], r["M"])
            assert int(g.s) == int(want_after[j])
        worst = max(worst, reservoirs_equal(got, want))
    within("numpy resample ulp", worst, RESAMPLE_ULP)


# ---- the numpy second readings: make_sky_fixture.py's float32 sky --------------------------------------------------------------------
def test_numpy_sky_reading(kat):
    miss = _load("make_sky_fixture").make(np.float32)
    n_hard = int(kat["sky_counts"][1])  # the rays with the miss shader's ray length and white light
    got = np.array([miss(kat["sky_origin"][j], kat["sky_dir"][j], kat["sky_sun"][j])[0] for j in range(n_hard)], F)
    within("make_sky_fixture float32 rel", rel(got, kat["sky_color"][:n_hard]), NUMPY_SKY_REL)


# ---- the numpy second readings: ibl_reference.py ---------------------------------------------------------------------------------------
def test_ibl_reference_reading(kat):
    import ibl_reference as ib

    x, y = ib.hammersley2d(kat["ham_i"], 1)
    assert same_bits(y, kat["ham_out"][:, 1]).all()
    for n in (32, 64):  # the first coordinate divides by N, which ibl_reference takes as one number
        m = kat["ham_N"] == n
        assert m.any() and same_bits(ib.hammersley2d(kat["ham_i"][m], n)[0], kat["ham_out"][m, 0]).all()
    rnd = ib.random2(kat["rnd_co"][:, 0], kat["rnd_co"][:, 1])
    N = kat["is_normal"]
    # random(normal.xz) is taken from the recording, so that the sine's 43758-fold error stays out of this comparison
    got = ib.importance_sample_ggx(kat["is_xi"][:, 0], kat["is_xi"][:, 1], kat["is_rough"], N, kat["is_rnd"])
    within("ibl random abs", float(np.abs(rnd.astype(np.float64) - kat["rnd_out"]).max()), IBL_RANDOM_ABS)
    within("ibl importanceSample_GGX ulp", int(ulps(got, kat["is_out"]).max()), IBL_GGX_ULP)


# ---- the numpy second readings: the per-light term of deferred and forward ----------------------------------------------------------
def _one_pixel_view(eye, num_lights=1):
    v = rr.types.ViewUniformData()
    v.eye_pos[:] = [float(x) for x in eye]
    v.num_lights, v.raytracing_supported, v.ssao_enabled = num_lights, 0, 0
    v.sun_dir[:] = [0.0, 1.0, 0.0]
    return v


def shading_term_distance(kat, monkeypatch, term):
    """largest ulp distance between a reading's per-light term and the recorded surfaceShading over the fixture's vectors with
    lightColorFactor 1 (what deferred.frag and forward.frag pass). The sun record that both readings put first is left out"""
    import hybrid_frame_reference as fr

    records = fr.light_records
    monkeypatch.setattr(fr, "light_records", lambda view, lights: records(view, lights)[1:])
    worst = 0
    use = np.flatnonzero(kat["ss_factor"] == 1.0)
    for j in use:
        got = term(kat["ss_pixel"][j], light_struct(kat["ss_light"][j]), _one_pixel_view(kat["ss_eye"][j]))
        worst = max(worst, int(ulps(got, kat["ss_out"][j]).max()))
    return worst


def test_deferred_term_reading(kat, monkeypatch):
    import hybrid_frame_reference as fr

    def term(px, light, view):
        # one G-buffer texel: occlusion 0 removes the ambient term, a white albedo makes baseColor the material's factor
        g = dict(position=np.array([[[*px[0:3], 1.0]]], F), normal=np.array([[[*px[6:9], 0.0]]], F), pbr=np.array([[[px[9], px[10], 0.0, 0.0]]], F),
                 albedo=np.full((1, 1, 4), 255, np.uint8))
        mesh = dict(metallic=1.0, roughness=1.0, type=0.0, base_color=px[3:6])
        return fr.deferred(g, None, None, None, view, [mesh], [light])[0, 0, :3]

    within("deferred term ulp", shading_term_distance(kat, monkeypatch, term), SHADING_TERM_ULP)


def test_deferred_glue_runs_over_the_reference_term(kat, monkeypatch):
    """deferred(surface_shading=) hands the callable what surfaceShading takes: with the recorded value returned, the glue adds
    nothing to it"""
    import hybrid_frame_reference as fr

    seen = {}

    def recorded(P, base, N, metallic, roughness, light, eye):
        seen.update(P=P, base=base, N=N, metallic=metallic, roughness=roughness, light=light, eye=eye)
        return kat["ss_out"][j][None, :]

    for j in (40, 41, 42, 43):
        px = kat["ss_pixel"][j]
        g = dict(position=np.array([[[*px[0:3], 1.0]]], F), normal=np.array([[[*px[6:9], 0.0]]], F), pbr=np.array([[[px[9], px[10], 0.0, 0.0]]], F),
                 albedo=np.full((1, 1, 4), 255, np.uint8))
        mesh = dict(metallic=1.0, roughness=1.0, type=0.0, base_color=px[3:6])
        monkeypatch.setattr(fr, "light_records", (lambda orig: lambda view, lights: orig(view, lights)[1:])(fr.light_records))
        out = fr.deferred(g, None, None, None, _one_pixel_view(kat["ss_eye"][j]), [mesh], [light_struct(kat["ss_light"][j])], surface_shading=recorded)
        monkeypatch.undo()
        assert ulps(out[0, 0, :3], kat["ss_out"][j]).max() == 0  # 0 + Lo: a negative zero of the term becomes +0
        assert same_bits(seen["light"], kat["ss_light"][j]).all() and same_bits(seen["P"][0], px[0:3]).all() and same_bits(seen["base"][0], px[3:6]).all()
        assert same_bits(seen["N"][0], px[6:9]).all() and same_bits(seen["eye"], kat["ss_eye"][j]).all()
        assert same_bits([seen["metallic"][0], seen["roughness"][0]], px[9:11]).all()


def test_forward_term_reading(kat, monkeypatch):
    import forward_reference as fw
    import hybrid_reference as hr

    def term(px, light, view):
        P, eye = px[None, 0:3], np.array(view.eye_pos[:], F)
        return fw.direct_lighting(P, px[None, 6:9], hr.normalize(eye[None, :] - P), px[None, 3:6], px[None, 9], px[None, 10], view, [light])[0]

    within("forward term ulp", shading_term_distance(kat, monkeypatch, term), SHADING_TERM_ULP)


# ---- whole passes over the recorded launches (the GPU tests of tests/test_gpu_ref_shaders.py run the same checks on the device) -----
W, H = 16, 8

def initial_ris_renderer(r, kat, count):
    for row in kat["lights"][:count]:
        r.add_gpu_light(light_struct(row))
    # some geometry so that the acceleration structure can be built (the passes below never cast a ray)
    v = np.zeros(3, dtype=VERTEX_DTYPE)
    v["pos"][:, :3] = [(50, 50, 50), (51, 50, 50), (50, 51, 50)]
    v["pos"][:, 3] = 1
    v["normal"][:, 2] = 1
    r.add_mesh(v, np.uint32([0, 1, 2]), rr.make_material(diffuse_map=r.default_diffuse_map()), None)
    r.initialize_raytracing()
    r.write_gbuffer_position(kat["gris_gbuffer"])
    return r


def initial_ris(r, count, frame):
    view = rr.types.ViewUniformData()
    view.num_lights, view.max_num_lights_used = count, 1024
    view.samples_per_frame, view.time = 1, 0.0
    view.total_samples = int(frame)  # the raygens' frame number: int(float(total_samples) + time * 10000)
    r.render_frame(view, rr.types.PASS_RESET_RESERVOIRS | rr.types.PASS_INITIAL_RIS)
    return r.read_reservoirs(0).reshape(-1)


def check_initial_ris(make, kat, ci):
    count = (1, 3, 1024)[ci]
    r = initial_ris_renderer(make(), kat, count)
    assert int(kat["gris_frame_drawing_one"][0]) == 4120 and 4120 in kat["gris_frames"]
    for fi, frame in enumerate(kat["gris_frames"]):
        got, want = initial_ris(r, count, frame), kat["gris_res"][ci, fi]
        assert np.array_equal(got["Y"], want["Y"]) and np.array_equal(got["M"], want["M"]), (count, frame)
        u = max(int(ulps(got["W_sum"], want["W_sum"]).max()), int(ulps(got["W_X"], want["W_X"]).max()))
        print(f"initial RIS, {count} lights, frame {frame}: {u} ulp")
        assert u <= RESAMPLE_ULP, (count, frame, u)
        assert (want["Y"] >= 0).any()



def check_sky(make, kat, case, margin):
    gen = _load("make_ref_shader_kat")
    scene, view = gen.sky_view(case)
    # the recorded rays are those of this view: jitter from the RNG (bit-exact to the compiled text, see above), then primary_ray
    view.total_samples = 1
    rays = []
    for i in range(W * H):
        (jx, jy), _ = oa.random_floats(oa.init_rng(i % W, i // W, W, oa.frame_number(view)), 2)
        rays.append(oa.primary_ray(view, W, H, i % W, i // W, float(jx), float(jy)))
    assert same_bits(np.array(rays, F), kat["gsky_rays"][case]).all()
    view.total_samples = 0
    r = scene.upload(make())
    rr.FrameLoop(r, scene.make_view(W, H, num_bounces=0, samples_per_frame=1, sky_enabled=1)).frame(rr.PASS_REFERENCE_PT)
    assert not r.read_accumulation()[..., :3].any(), "num_bounces = 0 traces nothing"
    r.reset_accumulation()
    rr.FrameLoop(r, view).frame(rr.PASS_REFERENCE_PT)
    got = r.read_accumulation()[..., :3].reshape(-1, 3)
    want = np.minimum(kat["gsky_color"][case], F(1.0))
    scale = np.maximum(np.abs(want).max(axis=1), 1e-9)
    err = float((np.abs(got.astype(np.float64) - want).max(axis=1) / scale).max())
    print(f"sky case {case}: relative distance {err:.3e}, clamped pixels {(kat['gsky_color'][case] > 1).any(axis=1).sum()}")
    assert np.isfinite(got).all() and err <= margin, err
    if case == 1:
        assert (kat["gsky_color"][case] > 1).any() and (got == 1.0).any()


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_oracle_initial_ris_pass(kat, ci):
    """the oracle's reset and initial-RIS passes on the recorded 16 x 8 launch: see test_gpu_ref_shaders.test_initial_ris"""
    check_initial_ris(lambda: oa.OracleRenderer(W, H), kat, ci)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_oracle_sky_pass(kat, case):
    """the oracle's path tracer on an empty scene against the recorded IntegrateScattering: see test_gpu_ref_shaders.test_sky"""
    check_sky(lambda: oa.OracleRenderer(W, H), kat, case, SKY_REL)

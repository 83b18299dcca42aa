"""CPU: the numpy restatement of one-bounce ray-traced diffuse GI (tests/rtgi_reference.py) held to known answers and properties on the
oracle's own G-buffer - a bare floor under the furnace, the inside of a closed box, an emissive wall, the courtyard (where it also proves
that the inputs of test_gpu_rtgi.py are adequate), the filter, the composite and the order of the per-pixel sum; and the proofs that the inputs of
test_gpu_walk_chunks.py (frames at which the persistent walks refill) and test_gpu_rtgi_scenes.py (the synthetic and the turned scene) are
adequate. test_gpu_rtgi.py holds the device to the restatement and runs the known answers there."""
import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rtgi_reference as gi

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

W, H = gi.W, gi.H
F = np.float32


def world(scene, width=W, height=H, defaults=True):
    """the scene on the oracle, its meshes as uploaded, its view and the oracle's G-buffer of it"""
    cpu = oa.OracleRenderer(width, height)
    meshes = hr.upload_recorded(scene, cpu, defaults)
    view = gi.scene_view(scene, width, height)
    return cpu, meshes, view, hr.gbuffer(cpu, meshes, view, width, height)


@pytest.fixture(scope="module")
def courtyard():
    return world(gi.courtyard_scene())


@pytest.fixture(scope="module")
def courtyard_rays(courtyard):
    """the courtyard's rays at 3 and at 16 samples, shared"""
    cpu, meshes, view, g = courtyard
    return {s: gi.gather(cpu, meshes, g, view, gi.default_params(samples=s)) for s in (3, 16)}


def test_the_rays_are_not_rtaos_own(courtyard):
    import rtao_reference as ao

    _, _, view, g = courtyard
    rows, nn, d = gi.directions(g, view, 4)
    rows_ao, _, d_ao = ao.directions(g, view, 4)
    assert np.array_equal(rows, rows_ao) and len(rows) > 1000 and np.isfinite(d).all()
    assert not np.array_equal(d, d_ao) and (d != d_ao).any(axis=-1).mean() > 0.99
    assert (hr.dot(d, np.broadcast_to(nn[:, None, :], d.shape)) >= 0).all()


def test_a_bare_floor_under_the_furnace_receives_exactly_one():
    cpu, meshes, view, g = world(gi.floor_scene())
    for samples in (1, 3, 16):
        p = gi.default_params(samples=samples, blur_radius=0)
        counts, E, cast, totals, _ = gi.gather(cpu, meshes, g, view, p, furnace=True)
        assert cast.any() and not cast.all()
        assert (counts[cast] == (0, 0, 0, samples)).all() and not counts[~cast].any()
        assert (E[cast] == 1.0).all() and not E[~cast].any()
        assert totals == (cast.sum(), samples * cast.sum(), 0, samples * cast.sum())
        Ef = gi.filter(g, E, gi.default_params(samples=samples, blur_radius=6))
        assert (Ef[cast] == 1.0).all() and not Ef[~cast].any()
    # without the furnace the same rays bring the sky: every count the same, E positive and finite
    counts2, E2, _, _, _ = gi.gather(cpu, meshes, g, view, gi.default_params(samples=3))
    assert (counts2[cast] == (0, 0, 0, 3)).all() and np.isfinite(E2).all() and (E2[cast] > 0).all()


def test_inside_a_closed_box_nothing_arrives():
    cpu, meshes, view, g = world(gi.inward_box_scene())
    for samples in (1, 8):
        p = gi.default_params(samples=samples)
        counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, p)
        assert cast.all() and (counts == (0, samples, 0, 0)).all() and not E.any()
        assert totals[0] == W * H and totals[1] == samples * W * H and totals[3] == 0
        # the sun is nearly overhead: rays that meet the floor would be lit but for the ceiling; those that meet the ceiling face away
        assert r["shadowed"].any() and (~r["shadowed"]).any() and totals[2] == r["shadowed"].sum()
        Ef = gi.filter(g, E, gi.default_params(samples=samples, blur_radius=6))
        assert not Ef[..., :3].any() and (Ef[..., 3] == 1).all()
        # under the furnace a hit brings nothing either, and casts no sun ray
        counts_f, E_f, _, totals_f, _ = gi.gather(cpu, meshes, g, view, p, furnace=True)
        assert (counts_f == (0, samples, 0, 0)).all() and not E_f.any() and totals_f[2] == 0


@pytest.mark.parametrize("max_radiance", [16.0, 0.5])
def test_an_emissive_wall_lights_the_wall_it_faces(max_radiance):
    cpu, meshes, view, g = world(gi.emissive_box_scene())
    assert [m["type"] for m in meshes] == [0.0, 3.0]
    samples = 16
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, gi.default_params(samples=samples, max_radiance=max_radiance))
    assert cast.all() and (g["position"][..., 2] < -1.19).all(), "every pixel is the wall that faces the emitter"
    assert (counts.sum(axis=-1) == samples).all() and not counts[..., gi.SUNLIT].any() and not counts[..., gi.MISSED].any()
    cap = F(min(gi.EMISSION, max_radiance))
    assert (E >= 0).all() and (E <= cap).all()
    lit = counts[..., gi.EMITTER] > 0
    print(f"{lit.mean():.3f} of the pixels have a ray that meets the emitter, at most {counts[..., gi.EMITTER].max()} of {samples}")
    assert lit.mean() > 0.5 and (E[lit] > 0).all() and not E[~lit].any()
    # a ray that meets the emitter brings min(emission, max_radiance) on every channel, every other ray of this box nothing
    want = counts[..., gi.EMITTER].astype(np.float32) * cap / F(samples)
    assert np.allclose(E, want[..., None], rtol=1e-6, atol=0)
    # no sun ray from an emitter hit: the sun rays are those of the other hits whose normal faces the sun
    assert totals[2] <= (r["kind"] == gi.DARK).sum()


def test_the_courtyard_is_an_adequate_input(courtyard, courtyard_rays):
    """conditions, not measurements: test_gpu_rtgi.py relies on them. At 3 and at 16 samples a quarter of the pixels that cast have no
    missed ray (the device must match them bit for bit), a tenth have a sunlit hit, a tenth a hit that is dark because its sun ray was
    occluded (not because NdotL is 0), a tenth a miss"""
    _, _, _, g = courtyard
    for samples, (counts, E, cast, totals, r) in courtyard_rays.items():
        k = r["kind"]
        no_miss, sunlit = (~(k == gi.MISSED).any(axis=1)).mean(), (k == gi.SUNLIT).any(axis=1).mean()
        shadowed, missed = r["shadowed"].any(axis=1).mean(), (k == gi.MISSED).any(axis=1).mean()
        print(f"{samples} samples, {len(r['rows'])} pixels: no missed ray {no_miss:.3f}, a sunlit hit {sunlit:.3f}, an occluded sun ray {shadowed:.3f}, a miss {missed:.3f}")
        assert cast.any() and not cast.all(), "the sky shows through the opening"
        assert no_miss >= 0.25 and sunlit >= 0.1 and shadowed >= 0.1 and missed >= 0.1
        assert (counts[cast].sum(axis=-1) == samples).all() and not counts[~cast].any()
        assert totals[2] == (k == gi.SUNLIT).sum() + r["shadowed"].sum() and totals[3] == (k == gi.MISSED).sum()
        assert np.isfinite(E).all() and (E >= 0).all() and (E <= 16.0).all()
    # uv matters: the sunlit hits on the checkered floor bring more than one albedo
    L = courtyard_rays[16][4]["L"][courtyard_rays[16][4]["kind"] == gi.SUNLIT]
    assert len(np.unique((L[:, 0] / L[:, 2]).round(2))) > 3
    # the red wall leaves a trace: where E is not grey, red leads somewhere on the floor
    E16, counts16 = courtyard_rays[16][1], courtyard_rays[16][0]
    floor = (g["pbr"][..., 3] == 0) & (counts16[..., gi.MISSED] == 0) & (counts16[..., gi.SUNLIT] > 0)
    assert floor.any() and (E16[floor][:, 0] > E16[floor][:, 2]).any()


def test_the_filter(courtyard, courtyard_rays):
    _, _, _, g = courtyard
    counts, E, cast, _, _ = courtyard_rays[3]
    # radius 0 is E itself, w = 1 where the pixel cast
    Ef0 = gi.filter(g, E, gi.default_params(blur_radius=0))
    assert np.array_equal(Ef0[..., :3], E) and np.array_equal(Ef0[..., 3] == 1, cast) and not Ef0[~cast].any()
    # thresholds nothing passes leave the centre tap alone
    assert np.array_equal(gi.filter(g, E, gi.default_params(blur_radius=6, blur_normal_cos=2.0)), Ef0)
    # taps across the wall / floor edge are rejected: give the floor 1 and everything else 0, and the floor stays exactly 1 and the
    # walls exactly 0 at every radius, though their pixels are neighbours
    floor = (g["pbr"][..., 3] == 0) & cast
    wall = (g["pbr"][..., 3] == 1) & cast
    touching = floor[1:, :] & wall[:-1, :]
    assert touching.any(), "floor pixels lie directly below pixels of the back wall"
    step = np.where(floor[..., None], F(1.0), F(0.0)) * np.ones(3, np.float32)
    for r in (1, 3, 6):
        Ef = gi.filter(g, step, gi.default_params(blur_radius=r))
        assert (Ef[floor][:, :3] == 1.0).all() and not Ef[wall][:, :3].any(), r
    # let every tap in and the edge blurs
    Ef = gi.filter(g, step, gi.default_params(blur_radius=1, blur_normal_cos=-1.0, blur_plane=np.inf))
    assert ((Ef[floor][:, 0] < 1.0).any()) and (Ef[wall][:, 0] > 0.0).any()
    # the window is [-r, r]^2, dy outer: an interior floor pixel at r = 1 is the ordered mean of its nine taps
    inner = floor.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(np.roll(floor, dy, axis=0), dx, axis=1)
    inner[[0, -1], :] = inner[:, [0, -1]] = False
    y, x = np.argwhere(inner)[0]
    Ef = gi.filter(g, E, gi.default_params(blur_radius=1))
    total = np.zeros(3, np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            total = total + E[y + dy, x + dx]
    assert np.array_equal(Ef[y, x, :3], total / F(9.0))
    # the flag a tap carries reaches exactly the pixels whose window counts it
    missed = counts[..., gi.MISSED] > 0
    _, tainted = gi.filter(g, E, gi.default_params(blur_radius=3), flag=missed)
    assert (tainted >= (missed & cast)).all() and tainted.sum() > missed.sum() and not tainted.all()


def test_the_filter_on_frames_smaller_than_its_window():
    for w, h in ((5, 3), (64, 1), (129, 2)):
        g = dict(position=np.ones((h, w, 4), np.float32), normal=np.tile(np.float32([0, 1, 0, 1]), (h, w, 1)))
        E = np.random.default_rng(w).random((h, w, 3), np.float32)
        Ef = gi.filter(g, E, gi.default_params(blur_radius=6))
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
            total = np.zeros(3, np.float32)
            taps = [(yy, xx) for yy in range(y - 6, y + 7) for xx in range(x - 6, x + 7) if 0 <= yy < h and 0 <= xx < w]
            for yy, xx in taps:
                total = total + E[yy, xx]
            assert np.array_equal(Ef[y, x, :3], total / F(len(taps))), (w, h, y, x)


def test_the_composite(courtyard, courtyard_rays):
    _, meshes, view, g = courtyard
    _, E, cast, _, _ = courtyard_rays[3]
    Ef = gi.filter(g, E, gi.default_params())
    rng = np.random.default_rng(3)
    deferred = rng.random((H, W, 4), np.float32)
    ssao = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    # intensity 0 adds exactly 0
    out, touched = gi.composite(g, ssao, deferred, Ef, view, meshes, 0.0)
    assert np.array_equal(out, deferred) and np.array_equal(touched, cast)
    out, _ = gi.composite(g, ssao, deferred, Ef, view, meshes, 1.0)
    assert np.array_equal(out[..., 3], deferred[..., 3]) and np.array_equal(out[~cast], deferred[~cast])
    assert (out[cast][:, :3] >= deferred[cast][:, :3]).all() and (out[cast][:, :3] > deferred[cast][:, :3]).any()
    # one pixel by hand: (((base (1 - metallic)) Ef) intensity) occlusion ssao / 65535
    y, x = np.argwhere(cast & (Ef[..., :3].sum(axis=-1) > 0))[0]
    m = meshes[int(g["pbr"][y, x, 3])]
    base = fr.gamma_table()[g["albedo"][y, x, :3]] * m["base_color"]
    add = ((base * (F(1.0) - g["pbr"][y, x, 0] * m["metallic"])) * Ef[y, x, :3]) * F(1.0)
    add = add * g["pbr"][y, x, 2]
    add = add * (F(ssao[H - 1 - y, x]) / F(65535.0))
    assert np.array_equal(out[y, x, :3], deferred[y, x, :3] + add)
    # without ssao_enabled the texel does not enter
    off = gi.scene_view(gi.courtyard_scene(), ssao_enabled=0)
    out_off, _ = gi.composite(g, ssao, deferred, Ef, off, meshes, 1.0)
    assert (out_off[cast][:, :3] >= out[cast][:, :3]).all() and not np.array_equal(out_off, out)
    # metal pixels hold their reflection under raytracing_supported == 1 and are left as they are; without it they receive
    metal = [dict(m, type=1.0) if i == 0 else m for i, m in enumerate(meshes)]
    floor = (g["pbr"][..., 3] == 0) & cast
    out_m, touched_m = gi.composite(g, ssao, deferred, Ef, view, metal, 1.0)
    assert floor.any() and np.array_equal(out_m[floor], deferred[floor]) and not touched_m[floor].any()
    assert np.array_equal(out_m[~floor], out[~floor])
    no_rt = gi.scene_view(gi.courtyard_scene(), raytracing_supported=0)
    assert np.array_equal(gi.composite(g, ssao, deferred, Ef, no_rt, metal, 1.0)[0], out)


def test_the_sum_is_in_sample_order(courtyard_rays):
    """float addition does not associate: exchanging two samples of different radiance changes E somewhere, so an unordered sum on the
    device would not pass test_gpu_rtgi.py"""
    L = courtyard_rays[16][4]["L"]
    E = gi.mean(L)
    # by hand, left to right
    k = int(np.argmax((L[:, :, 0] > 0).sum(axis=1)))
    acc = L[k, 0]
    for s in range(1, 16):
        acc = acc + L[k, s]
    assert np.array_equal(E[k], acc / F(16.0))
    swapped = L.copy()
    swapped[:, [0, 15]] = swapped[:, [15, 0]]
    Es = gi.mean(swapped)
    differ = (E != Es).any(axis=1)
    print(f"exchanging samples 0 and 15 changes E of {differ.sum()} of {len(E)} pixels")
    assert differ.any() and np.allclose(E, Es, rtol=1e-5, atol=1e-7)
    assert not differ[(L[:, 0] == L[:, 15]).all(axis=1)].any()


def test_the_clamp_maps_nan_negatives_and_minus_zero_to_plus_zero():
    x = np.array([np.nan, -1.0, -0.0, 0.0, 0.25, 16.0, 17.0, np.inf], np.float32)
    got = gi.clamp(x, 16.0)
    assert np.array_equal(got, np.float32([0, 0, 0, 0, 0.25, 16, 16, 16])) and not np.signbit(got).any()


# ---- the inputs of test_gpu_walk_chunks.py ----------------------------------------------------------------------------------------
LANES = gi.WALK_LANES


def test_the_boxes_of_the_refill_tests_are_adequate():
    """conditions test_gpu_walk_chunks.py relies on: at their frames every pixel of the two boxes casts and no ray misses (every pixel is
    bit for bit), the closed box has 3 grids of rays, the emissive box 2 at three samples with a partial last chunk, and RTAO's box 3"""
    import rtao_reference as ao

    w, h = gi.WALK_BOX_SIZE
    cpu, meshes, view, g = world(gi.inward_box_scene(), w, h)
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, gi.default_params(samples=16))
    assert cast.all() and (counts == (0, 16, 0, 0)).all() and totals[:2] == (w * h, 16 * w * h) and totals[3] == 0 and totals[1] >= 3 * LANES
    assert 0 < totals[2] < LANES, "the sun rays of this box stay within one grid: the courtyard refills k_rtgi_shadow"
    w, h = gi.WALK_EMISSIVE_SIZE
    cpu, meshes, view, g = world(gi.emissive_box_scene(), w, h)
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, gi.default_params(samples=3, max_radiance=0.5))
    assert cast.all() and totals[3] == 0 and not counts[..., gi.SUNLIT].any() and 2 * LANES <= totals[1] < 3 * 2 * LANES and totals[1] % 64 != 0
    lit = counts[..., gi.EMITTER] > 0
    assert 0.25 < lit.mean() < 1 and np.array_equal(E, np.repeat((counts[..., gi.EMITTER] * F(0.5) / F(3.0))[..., None], 3, axis=-1))
    w, h = gi.WALK_AO_SIZE
    cpu, meshes, view, g = world(ao.inward_box_scene(), w, h)
    count, totals = ao.counts(cpu, g, view, ao.MAX_SAMPLES, ao.BOX_RADIUS)
    assert totals == (w * h, 64 * w * h, 64 * w * h) and totals[1] >= 3 * LANES and (count == 64).all()


def yard_totals(width, height):
    cpu, meshes, view, g = world(gi.courtyard_scene(), width, height)
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, gi.default_params(samples=16))
    return totals, r


def test_the_courtyard_of_the_refill_tests_is_adequate_and_the_smallest_of_its_family():
    """at WALK_YARD_SIZE and 16 samples the courtyard casts two grids of sun rays (k_rtgi_shadow refills twice), some of them occluded,
    and some rays miss; the next smaller frame of its family (odd widths, heights the nearest odd number to 41 / 67 of the width) does
    not reach two grids. Measured: 20,001 pixels, 320,016 rays, 134,390 sun rays, 25,479 misses; 181 x 111 gives 130,870 sun rays"""
    w, h = gi.WALK_YARD_SIZE
    totals, r = yard_totals(w, h)
    print(totals)
    assert totals[1] >= 3 * LANES and totals[2] >= 2 * LANES and totals[3] > 0
    assert (r["kind"] == gi.SUNLIT).sum() > 0 and r["shadowed"].sum() > 0 and totals[3] < 0.1 * totals[1]
    smaller = (w - 2, int(round((w - 2) * 41 / 67)) | 1)
    assert yard_totals(*smaller)[0][2] < 2 * LANES, smaller


# ---- the inputs of test_gpu_rtgi_scenes.py ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [3, 16])
def test_the_synthetic_scene_is_an_adequate_input(samples):
    """hybrid_util.synthetic_scene at 67 x 41: metal pixels that cast, pixels that are no metal with metallic and occlusion texels that
    enter the composite, rays on all four meshes; and the side of the composite the device never shows: without raytracing_supported
    the metal pixels receive too (the pass refuses such a view, so only the restatement has it)"""
    from hybrid_util import synthetic_scene

    cpu, meshes, view, g = world(synthetic_scene(), defaults=False)
    assert view.raytracing_supported == 1 and [m["type"] for m in meshes] == [1.0, 0.0, 0.0, 1.0]
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, gi.default_params(samples=samples))
    material = g["pbr"][..., 3].astype(np.uint32)
    geo = g["position"][..., 3] != 0
    typ = np.array([m["type"] for m in meshes], np.float32)[np.minimum(material, 3)]
    mf = np.array([m["metallic"] for m in meshes], np.float32)[np.minimum(material, 3)]
    metal, matte = geo & (typ == 1.0), geo & (typ != 1.0) & cast
    assert metal.sum() >= 100 and cast[metal].all()
    assert (matte & (g["pbr"][..., 0] * mf != 0)).sum() >= 20 and (matte & (g["pbr"][..., 2] != 1)).sum() >= 20
    assert all((r["mesh"] == i).sum() >= 10 for i in range(4)) and r["flipped"].any()
    assert not np.array_equal(g["normal"][metal][:, :3], np.tile(np.float32([0, 1, 0]), (metal.sum(), 1))), "the floor's normals come from its normal map"
    Ef = gi.filter(g, E, gi.default_params(blur_radius=0))
    deferred = np.random.default_rng(5).random((H, W, 4), np.float32)
    ssao = np.full((H, W), 65535, np.uint16)
    out, touched = gi.composite(g, ssao, deferred, Ef, view, meshes, 1.0)
    assert not touched[metal].any() and np.array_equal(out[metal], deferred[metal]) and touched[matte].all()
    no_rt = gi.scene_view(synthetic_scene(), raytracing_supported=0)
    out0, touched0 = gi.composite(g, ssao, deferred, Ef, no_rt, meshes, 1.0)
    assert touched0[metal].all() and (out0[metal][:, :3] >= deferred[metal][:, :3]).all() and np.array_equal(out0[matte], out[matte])
    # metallic below 1 lets some of it through: the floor's metallic texel times the factor is not 1 everywhere
    assert (out0[metal][:, :3] > deferred[metal][:, :3]).any()


@pytest.mark.parametrize("samples", [3, 16])
def test_the_turned_scene_is_an_adequate_input(samples):
    """the counts test_gpu_rtgi_scenes.py asserts on the device's G-buffer, here on the oracle's: at least 50 rays meet a surface from
    behind (all of them the wall), 20 of them sunlit - which they are only because the normal was turned: before the turn it faces away
    from the sun - 20 rays on each of the metal, dielectric and type-4 meshes and on the mirrored box, 10 on the sheet of zero normals,
    all dark without a sun ray, and 10 sunlit rays on the panel whose colour the clamp maps to (+0, max_radiance, +0)"""
    cpu, meshes, view, g = world(gi.turned_scene())
    M = gi.TURNED_MESHES
    assert [m["type"] for m in meshes] == [0.0, 0.0, 0.0, 1.0, 2.0, 4.0, 0.0, 0.0]
    w = meshes[M["mirrored"]]["world"]
    assert np.linalg.det(np.asarray(w, np.float64).reshape(3, 4)[:, :3]) < 0, "the mirrored instance"
    uv = meshes[M["wall"]]["vertices"]["uv"]
    assert uv.min() < 0 and uv.max() > 1
    p = gi.default_params(samples=samples)
    counts, E, cast, totals, r = gi.gather(cpu, meshes, g, view, p)
    k, flipped = r["kind"], r["flipped"]
    print({name: int((r["mesh"] == i).sum()) for name, i in M.items()}, "flipped", int(flipped.sum()), "of them sunlit", int((flipped & (k == gi.SUNLIT)).sum()))
    assert flipped.sum() >= 50 and (flipped & (k == gi.SUNLIT)).sum() >= 20 and (flipped & (r["mesh"] == M["wall"])).sum() >= 50
    sun = hr.sun_direction(view)
    turned = flipped & (k == gi.SUNLIT)
    assert (hr.dot(r["Nh"][turned], np.broadcast_to(sun, r["Nh"][turned].shape)) > 0).all(), "lit after the turn"
    assert (hr.dot(-r["Nh"][turned], np.broadcast_to(sun, r["Nh"][turned].shape)) < 0).all(), "and not before it"
    for name in ("metal", "dielectric", "pbr", "mirrored"):
        assert (r["mesh"] == M[name]).sum() >= 20, name
    assert ((r["mesh"] == M["mirrored"]) & (k == gi.SUNLIT)).sum() >= 10
    zero = r["mesh"] == M["zero"]
    assert zero.sum() >= 10 and (k[zero] == gi.DARK).all() and not r["shadowed"][zero].any() and np.isnan(r["Nh"][zero]).all()
    assert totals[2] == (k == gi.SUNLIT).sum() + r["shadowed"].sum()
    clamp = (r["mesh"] == M["clamp"]) & (k == gi.SUNLIT)
    assert clamp.sum() >= 10 and (r["L"][clamp] == (0.0, 16.0, 0.0)).all() and not np.signbit(r["L"][clamp]).any()
    visible = np.unique(g["pbr"][..., 3][g["position"][..., 3] != 0])
    assert M["zero"] not in visible and M["clamp"] not in visible and {M["wall"], M["metal"], M["dielectric"], M["pbr"], M["mirrored"]} <= set(visible.tolist())
    # the texture repeats: the sunlit hits on the wall bring both colours of its checker
    wall = r["L"][(r["mesh"] == M["wall"]) & (k == gi.SUNLIT)]
    assert len(np.unique((wall[:, 0] / wall[:, 2]).round(1))) >= 2
    assert np.isfinite(E).all() and (E >= 0).all()


def test_frame_numbers_that_wrap_give_other_rays():
    """(frame * 64 + s) ^ SEED_XOR in 32 bits: the views of test_gpu_rtgi_scenes.py's wrap test have the frame numbers it says, and their
    rays are neither frame 0's nor each other's"""
    scene = gi.turned_scene()
    cpu, meshes, view, g = world(scene)
    views = [view, gi.scene_view(scene, total_samples=2 ** 26 + 8), gi.scene_view(scene, time=-0.0001)]
    assert [oa.frame_number(v) for v in views] == [0, 2 ** 26 + 8, 2 ** 32 - 1]
    d = [gi.directions(g, v, 3)[2] for v in views]
    assert np.isfinite(d[1]).all() and np.isfinite(d[2]).all()
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[0], d[2]) and not np.array_equal(d[1], d[2])
    # 2^26 + 8 wraps onto frame 8: the same words, the same rays
    assert np.array_equal(d[1], gi.directions(g, gi.scene_view(scene, total_samples=8), 3)[2])

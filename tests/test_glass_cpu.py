"""CPU: the restatement of the ray-traced glass (tests/glass_reference.py) on its own - the event against float64 Snell and mirror
directions, with the normal on either side; the adequacy of the gallery on the oracle's G-buffer (the GPU test asserts it again on the
device's); the identities that define UhGlassStats; the nested boxes; the known answers that need no device."""
import numpy as np
import pytest

import glass_reference as gs

F = np.float32
# 64 incidence angles from 0.5 to 80 degrees. Beyond 80 degrees T is no longer within 1e-6 for a reason that is float32's, not the
# event's: k = 1 - eta^2 (1 - dn^2) carries an absolute error of about 6e-8, and sqrt(k) turns it into 6e-8 / (2 sqrt(k)), which passes
# 1e-6 once sqrt(k) < 0.03 (ior 1: 88 degrees). The grid's step, 1.26 degrees, also keeps its nearest angle 0.2 degrees from the critical
# angle of ior 0.6 (36.87 degrees), on the side where nothing is refracted.
ANGLES = np.radians(np.linspace(0.5, 80.0, 64))
N64 = np.array([0.3, 0.8, -0.52]) / np.linalg.norm([0.3, 0.8, -0.52])
T64 = np.cross(N64, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(N64, [0.0, 0.0, 1.0]))


def incident():
    """64 unit directions arriving at the surface with normal N64 at ANGLES from it, float64"""
    return np.sin(ANGLES)[:, None] * T64[None, :] - np.cos(ANGLES)[:, None] * N64[None, :]


@pytest.mark.parametrize("far_side", [False, True], ids=["normal toward the ray", "normal on the far side"])
@pytest.mark.parametrize("ior", [1.5, 1.0, 0.6])
def test_the_event_against_float64(ior, far_side):
    """T within 1e-6 of Snell with eta = 1 / ior, R the mirror direction, `cannot` wherever eta sin is 1e-5 or more away from 1, w0 + w1
    within 1 ulp of 1. A normal given on the far side is turned toward the ray first (rchit:35-37), as the pass turns Nn and every hit
    normal: the event then sees dnd <= 0 and takes eta = 1 / ior - the flip and the quirk - and gives the same bits"""
    d64 = incident()
    nd = d64.astype(np.float32)
    given = np.broadcast_to((-N64 if far_side else N64).astype(np.float32), nd.shape)
    N, flipped = gs.turn(given, nd)
    assert flipped.all() == far_side and flipped.any() == far_side
    e = gs.event(nd, N, np.full(len(nd), ior, np.float32))
    assert (e["ratio"] == F(1.0) / F(ior)).all(), "1 / ior whichever side the normal was given on"
    eta = 1.0 / ior
    nd64 = nd.astype(np.float64)
    nd64 /= np.linalg.norm(nd64, axis=1)[:, None]
    cos = -(nd64 @ N64)
    sin = np.sqrt(1.0 - cos * cos)
    decided = np.abs(eta * sin - 1.0) >= 1e-5
    assert decided.all(), "no angle of the grid is that close to the critical angle"
    assert np.array_equal(e["cannot"], eta * sin > 1.0)
    assert e["cannot"].any() == (ior < 1.0) and not e["cannot"].all()
    R64 = nd64 + 2.0 * cos[:, None] * N64[None, :]
    assert np.abs(e["R"] - R64).max() <= 1e-6
    ok = ~e["cannot"]
    k = 1.0 - eta * eta * (1.0 - cos * cos)
    T_snell = eta * nd64[ok] + (eta * cos[ok] - np.sqrt(k[ok]))[:, None] * N64[None, :]
    assert np.abs(e["T"][ok] - T_snell).max() <= 1e-6
    assert np.abs(np.linalg.norm(e["T"][ok].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    w0, w1 = np.where(e["cannot"], F(1.0), e["Fr"]), F(1.0) - e["Fr"]
    total = np.where(e["cannot"], w0, w0 + w1)  # with `cannot` chain 1 is not cast
    assert (np.abs(total.astype(np.float64) - 1.0) <= np.spacing(F(1.0))).all()
    assert ((e["Fr"] >= 0) & (e["Fr"] <= 1)).all()
    if far_side:
        near = gs.event(nd, np.broadcast_to(N64.astype(np.float32), nd.shape), np.full(len(nd), ior, np.float32))
        for key in ("R", "T", "Fr", "cannot"):
            assert np.array_equal(e[key].view(np.uint8), near[key].view(np.uint8)), key


def test_an_unturned_normal_gives_the_other_glass():
    """what the pass does not do: handed the far-side normal as it is, the event takes ratio = ior - textbook Snell for a ray that leaves
    the glass - and at ior 1.5 cannot refract beyond asin(1 / 1.5), where the reference's glass always refracts"""
    nd = incident().astype(np.float32)
    far = np.broadcast_to((-N64).astype(np.float32), nd.shape)
    e = gs.event(nd, far, np.full(len(nd), 1.5, np.float32))
    assert (e["ratio"] == F(1.5)).all() and e["cannot"].any()
    turned = gs.event(nd, gs.turn(far, nd)[0], np.full(len(nd), 1.5, np.float32))
    assert not turned["cannot"].any() and not np.array_equal(e["T"], turned["T"])


@pytest.fixture(scope="module")
def gallery():
    cpu, meshes, ior, v, g = gs.cpu_world(gs.gallery_scene(), *gs.GALLERY_SIZE)
    chains = {k: gs.chains(cpu, meshes, ior, g, v, gs.default_params(max_events=k)) for k in (1, 2, 8)}
    return dict(cpu=cpu, meshes=meshes, ior=ior, v=v, g=g, chains=chains)


def test_the_gallery_is_adequate_on_the_oracles_gbuffer(gallery):
    got = gs.assert_adequate(gallery["chains"][8], gallery["chains"][2])
    print(got, len(gallery["chains"][8]["px"]["rows"]), "casting pixels")
    types = {int(gallery["meshes"][i]["type"]) for i in range(len(gallery["meshes"]))}
    assert types == {0, 1, 2, 3}, "a lamp, a metal ball and glass beside the courtyard's Lambertian meshes"
    assert sorted(set(gallery["ior"][[gs.GALLERY_MESHES[k] for k in ("ball", "slab", "thin", "far_ball", "mirrored")]].tolist())) == [F(0.6), F(1.5)]
    world = gallery["meshes"][gs.GALLERY_MESHES["mirrored"]]["world"].reshape(3, 4)[:, :3]
    assert np.linalg.det(world.astype(np.float64)) < 0 and len({round(float(np.linalg.norm(world[:, k])), 3) for k in range(3)}) == 3, "mirrored, non-uniform"


@pytest.mark.parametrize("max_events", [1, 2, 8])
def test_the_identities_that_define_the_stats(gallery, max_events):
    ch = gallery["chains"][max_events]
    t, m = ch["totals"], len(ch["px"]["rows"])
    first_tir = int(ch["tir0"].sum())
    assert t["pixels"] == m and t["chains"] + first_tir == 2 * m
    assert t["segments"] == t["chains"] + t["events"] == sum(ch["rounds"])
    assert t["events"] == int((ch["events"].astype(np.int64) - 1)[ch["events"] > 0].sum()), "the events behind the first, over the cast chains"
    assert t["tir"] >= first_tir and t["cut"] == int(ch["cut"].sum()) and t["misses"] == int((ch["kind"] == gs.MISSED).sum())
    assert (ch["events"] <= max_events).all() and (ch["events"][ch["cut"]] == max_events).all()
    assert not ch["events"][:, 1][ch["tir0"]].any() and (ch["events"][:, 1][~ch["tir0"]] >= 1).all() and (ch["events"][:, 0] >= 1).all()
    _, counts, ev, cast, _ = gs.images(gallery["g"], ch, gs.default_params(max_events=max_events))
    assert (counts[cast].sum(axis=-1) == 2).all() and not counts[~cast].any() and not ev[~cast].any() and not ev[..., 3].any()
    assert np.array_equal((ev[..., 2] & gs.TIR) != 0, cast & (ev[..., 1] == 0))
    if max_events == 1:
        assert t["events"] == 0 and t["cut"] > 0 and ch["rounds"][1:] == []
    if max_events == 8:
        assert t["tir"] > first_tir, "refraction is impossible at some later event too (the ior-0.6 slab from inside)"


def test_with_one_event_a_chain_that_meets_glass_is_cut(gallery):
    """max_events = 1: chain 1 of the convex ball meets the ball's far side and is cut, so C = R_0 exactly; the TIR pixels' C is clamp(L_0)"""
    ch = gallery["chains"][1]
    p = gs.default_params(max_events=1)
    rad, counts, ev, cast, _ = gs.images(gallery["g"], ch, p)
    mat = gallery["g"]["pbr"][..., 3].astype(np.uint32).reshape(-1)[ch["px"]["rows"]]
    on_ball = mat == gs.GALLERY_MESHES["ball"]
    ball = on_ball & ch["cut"][:, 1]
    # (a few pixels on the icosphere's silhouette refract past its far side: their normals are interpolated, their facets are flat)
    print(on_ball.sum(), "pixels on the ball,", ball.sum(), "with chain 1 cut")
    assert ball.sum() >= 100 and ball.sum() >= 0.95 * on_ball.sum() and not ch["R"][ball, 1].any()
    C = rad.reshape(-1, 4)[ch["px"]["rows"]][:, :3]
    assert np.array_equal(C[ball].view(np.uint32), ch["R"][ball, 0].view(np.uint32))
    tir = ch["tir0"]
    assert (ch["weights"][tir, 0] == 1.0).all() and np.array_equal(C[tir].view(np.uint32), ch["R"][tir, 0].view(np.uint32))


def test_the_nested_boxes():
    """every pixel casts, chain 1 reaches the emitter after 2 events and chain 0 after 3, C = 1 to the last bit or the one before; at
    WALK_NESTED_SIZE round 0 and round 1 hold more rays than a persistent grid has lanes"""
    for size in ((gs.W, gs.H), gs.WALK_NESTED_SIZE):
        cpu, meshes, ior, v, g = gs.cpu_world(gs.nested_boxes_scene(), *size)
        ch = gs.chains(cpu, meshes, ior, g, v, gs.default_params())
        rad, counts, ev, cast, missed = gs.images(g, ch, gs.default_params())
        n = size[0] * size[1]
        assert cast.all() and not missed.any() and (counts == (0, 0, 2, 0)).all() and (ev == (3, 2, 0, 0)).all()
        assert ch["rounds"][:4] == [2 * n, 2 * n, n, 0] and ch["totals"]["tir"] == 0 and ch["totals"]["shadow_rays"] == 0
        assert (np.abs(rad[..., :3].astype(np.float64) - 1.0) <= np.spacing(F(1.0))).all()
    assert 2 * n == 87842 and 2 * n > gs.WALK_LANES


def test_the_courtyard_has_no_glass():
    cpu, meshes, ior, v, g = gs.cpu_world(gs.no_glass_scene())
    ch = gs.chains(cpu, meshes, ior, g, v, gs.default_params())
    assert not any(ch["totals"].values()) and ch["rounds"] == [0] * 8
    rad, counts, ev, cast, _ = gs.images(g, ch, gs.default_params())
    assert not rad.any() and not counts.any() and not ev.any() and not cast.any()


def test_under_the_furnace_an_open_scene_returns_one(gallery):
    """furnace, max_events = 16: every chain that is not cut ends on the sky or the lamp with L = 1 or on another surface with L = 0; where
    both chains end at 1, C = w0 + w1 is within 1 ulp of 1"""
    ch = gs.chains(gallery["cpu"], gallery["meshes"], gallery["ior"], gallery["g"], gallery["v"], gs.default_params(max_events=16), furnace=True)
    assert ch["totals"]["shadow_rays"] == 0
    bright = np.isin(ch["kind"], (gs.EMITTER, gs.MISSED))
    both = bright[:, 0] & (bright[:, 1] | ch["tir0"])
    assert both.sum() >= 100
    C = gs.clamp_sum(ch, 16.0)
    assert (np.abs(C[both].astype(np.float64) - 1.0) <= 1e-6).all()

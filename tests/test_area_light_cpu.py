"""CPU: the restatement of the hybrid frame's area lights (tests/area_light_reference.py, from DESIGN.md section 2 "Area lights") on the
oracle's G-buffer: the table's properties, the pick frequencies, a known answer (the irradiance under a parallel rectangle, in closed
form), a float64 restatement of the geometry lines, and the adequacy of the scenes the GPU tests use."""
import numpy as np
import pytest

import area_light_reference as al
import hybrid_reference as hr
import oracle_api as oa

W, H = al.W, al.H


class Cpu:
    def __init__(self, scene):
        self.scene = scene
        self.oracle = oa.OracleRenderer(W, H)
        self.meshes = hr.upload_recorded(scene, self.oracle)
        self.view = al.scene_view(scene)
        self.g = hr.gbuffer(self.oracle, self.meshes, self.view, W, H)
        self.tab = al.table(self.meshes)


@pytest.fixture(scope="module")
def room():
    return Cpu(al.room_scene())


@pytest.fixture(scope="module")
def three():
    return Cpu(al.three_lamp_scene())


@pytest.fixture(scope="module")
def three_samples(three):
    return al.samples(three.g, three.view, three.meshes, al.default_params(samples=16), three.tab)


@pytest.fixture(scope="module")
def room_gathered(room):
    return al.gather(room.oracle, room.meshes, room.g, room.view, al.default_params(samples=16), room.tab)


def test_rng_restatement_is_the_oracles():
    for px, py, frame in ((0, 0, 0), (5, 7, 3 * 64 + 2), (66, 40, (9 * 64 + 15) ^ al.SEED_XOR)):
        s = oa.init_rng(px, py, W, frame & 0xFFFFFFFF)
        assert int(al.init_rng(np.array([px]), np.array([py]), W, frame)[0]) == s
        want, _ = oa.random_floats(s, 3)
        state, got = np.array([s], np.uint64), []
        for _ in range(3):
            state, word = al.step(state)
            got.append(al.to_float(word)[0])
        assert np.array_equal(np.array(got, np.float32), want)


def test_table_properties(room, three):
    for w in (room, three):
        t = w.tab
        n = len(t["keys"])
        q, a = t["weights"].astype(np.float64), t["areas"].astype(np.float64)
        assert n > 0 and t["b"] == 31 - int(n - 1).bit_length()
        assert np.array_equal(q >= 1, a > 0), "q >= 1 exactly where the area is > 0"
        assert t["total"] == int(q.sum()) <= 1 << 31 and np.array_equal(t["cum"].astype(np.uint64), np.cumsum(t["weights"].astype(np.uint64)))
        big = int(np.argmax(a))
        assert 2.0 ** (t["b"] - 1) <= q[big] < 2.0 ** t["b"], "the largest triangle's weight lies in [2^(b-1), 2^b)"
        pos = a > 0
        ratio = q[pos] * a[big] / (a[pos] * q[big])
        bound = 1.0 + 1.0 / q[pos]
        print(f"{w.scene.name}: N {n} b {t['b']} x {t['x']} total {t['total']} weights {t['weights']} ratio in [{ratio.min():.9f}, {ratio.max():.9f}]")
        # q = trunc(s a) lies in (s a - 1, s a]: q_i / (s a_i) in (1 / (1 + 1 / q_i), 1], and likewise for the largest, whose q is no smaller
        assert (ratio <= bound).all() and (ratio >= 1.0 / bound).all(), "within the truncation bound, a factor of 1 + 1 / q_i either way"
    t = three.tab
    assert len(t["keys"]) == 6 and (t["areas"] == 0).sum() == 1, "scene 2: three emitter meshes, one degenerate triangle"
    assert t["areas"].max() / t["areas"][t["areas"] > 0].min() >= 1e4
    mirrored = three.meshes[(int(t["keys"][-1]) >> al.PRIM_BITS)]["world"]
    assert np.linalg.det(np.asarray(mirrored, np.float64).reshape(3, 4)[:, :3]) < 0, "one emitter under a mirrored instance"
    assert [int(k) >> al.PRIM_BITS for k in t["keys"]] == [3, 3, 4, 4, 5, 5] and [int(k) & ((1 << al.PRIM_BITS) - 1) for k in t["keys"]] == [0, 1, 0, 1, 0, 1]


def test_pick_frequencies_match_the_weights(three, three_samples):
    t = three.tab
    picks = three_samples["pick"].reshape(-1)
    n = len(picks)
    assert n >= 16 * 1500
    p = t["weights"].astype(np.float64) / t["total"]
    got = np.bincount(picks, minlength=len(p)).astype(np.float64)
    sigma = np.sqrt(n * p * (1 - p))
    print(f"{n} picks: got {got}, expected {n * p}, sigma {sigma}")
    assert (np.abs(got - n * p) <= 5 * sigma).all()
    # adequacy of scene 2 for the GPU tests: every emitter with area is picked, the degenerate one never
    assert (got[t["areas"] > 0] >= 1).all() and (got[t["areas"] == 0] == 0).all()


def _corner(a, b, h):
    """the form factor of a rectangle with a corner over the element, sides a and b at height h; odd in a and in b"""
    ra, rb = np.sqrt(h * h + a * a), np.sqrt(h * h + b * b)
    return (a / ra * np.arctan(b / ra) + b / rb * np.arctan(a / rb)) / (2.0 * np.pi)


def test_known_answer_irradiance_under_a_parallel_rectangle():
    half, height = (0.6, 0.4), 1.5
    w = Cpu(al.open_floor_scene(half, height))
    p = al.default_params(samples=16, blur_radius=0, max_weight=al.FLT_MAX, max_radiance=al.FLT_MAX)
    smp = al.samples(w.g, w.view, w.meshes, p, w.tab)
    P = w.g["position"][..., :3].reshape(-1, 3)[smp["rows"]].astype(np.float64)
    band = (np.abs(P[:, 0]) < 1.5) & (np.abs(P[:, 2]) < 1.0) & (np.abs(P[:, 1]) < 1e-3)
    assert band.sum() >= 100
    x = np.where(smp["away"], 0.0, smp["G"].astype(np.float64) * smp["NdotL"].astype(np.float64))[band]
    est = x.mean()
    se = np.sqrt((x.var(axis=1, ddof=1) / x.shape[1]).sum()) / x.shape[0]
    px, pz = P[band, 0], P[band, 2]
    form = (_corner(half[0] - px, half[1] - pz, height) - _corner(-half[0] - px, half[1] - pz, height)
            - _corner(half[0] - px, -half[1] - pz, height) + _corner(-half[0] - px, -half[1] - pz, height))
    want = (np.pi * form).mean()
    print(f"{band.sum()} floor pixels, 16 samples each: mean(G NdotL) {est:.6f}, closed form {want:.6f}, standard error {se:.6f}, off by {(est - want) / se:.2f} se")
    assert want > 0.1 and abs(est - want) <= 5 * se


def test_float64_restatement_bounds_the_geometry_lines(room, three):
    for w in (room, three):
        p = al.default_params(samples=16, max_weight=al.FLT_MAX)
        a32 = al.samples(w.g, w.view, w.meshes, p, w.tab)
        a64 = al.samples(w.g, w.view, w.meshes, p, w.tab, dtype=np.float64)
        assert np.array_equal(a32["pick"], a64["pick"]) and np.array_equal(a32["Y"], a64["Y"]), "integer picks, the same points"
        both = ~a32["away"] & ~a64["away"]
        flips = int((a32["away"] != a64["away"]).sum())
        t = w.tab
        P = w.g["position"][..., :3].reshape(-1, 3)[a32["rows"]].astype(np.float64)
        wv = a64["Y"].astype(np.float64) - P[:, None, :]
        scale = (t["areas"][a64["pick"]].astype(np.float64) * t["total"] / t["weights"][a64["pick"]].astype(np.float64)) / (wv * wv).sum(axis=-1)
        err = np.abs(a32["g0"].astype(np.float64) - a64["g0"])[both] / scale[both]
        print(f"{w.scene.name}: {both.sum()} samples, max |g0_32 - g0_64| / (invpdf / d2) {err.max():.3e}; {flips} samples away in one precision alone")
        assert err.max() <= 2e-5
        assert flips <= both.sum() // 1000


def test_scene_1_is_adequate_for_the_gpu_tests(room, room_gathered):
    counts, D, Sp, cast, emitter, totals, smp = room_gathered
    n = smp["away"].size
    lit, occ, away = counts[..., al.LIT].sum() / n, counts[..., al.OCCLUDED].sum() / n, counts[..., al.AWAY].sum() / n
    mixed = ((counts[..., al.LIT] > 0) & (counts[..., al.OCCLUDED] > 0)).sum()
    print(f"scene 1: {cast.sum()} pixels cast, lit {lit:.3f} occluded {occ:.3f} away {away:.3f}, {mixed} penumbra pixels, {emitter.sum()} emitter pixels, totals {totals}")
    assert lit >= 0.1 and occ >= 0.1 and away >= 0.05
    assert mixed >= 20, "penumbra"
    assert emitter.sum() >= 10, "emitter pixels in the frame"
    assert (counts[cast].sum(axis=-1) == 16).all() and not counts[~cast].any()
    assert np.isfinite(D).all() and np.isfinite(Sp).all() and D.max() > 0 and Sp.max() > 0


def test_no_emitter_no_pixel_casts():
    w = Cpu(al.dark_scene())
    assert w.tab["total"] == 0 and len(w.tab["keys"]) == 0
    deferred = np.random.default_rng(1).random((H, W, 4)).astype(np.float32)
    out = al.image(w.oracle, w.meshes, w.g, w.view, al.default_params(), deferred, w.tab)
    assert not out["cast"].any() and not out["emitter"].any() and not out["counts"].any() and not out["diffuse"].any() and not out["specular"].any()
    assert np.array_equal(out["deferred"], deferred)

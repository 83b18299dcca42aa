"""The float64 sampler of tests/texture_f64.py against the project's two float32 readings of the same sampler - the oracle's
(oracle.cpp sample_texture, through orc_sample_texture) and the numpy one of tests/forward_reference.py -, on the texture shapes and
the uv that tests/test_gpu_textures.py puts on the device. It shows that a correct float32 sampler stays within the bound the GPU test
holds the device to, and measures the one constant of that bound. Needs no GPU."""
import numpy as np
import pytest

import forward_reference as fw
import oracle_api as oa
import texture_f64 as tx

WIDEN = tx.WIDEN


def uv_samples(h, w, seed):
    """float32 (u, v): a few thousand uniform in [-3, 4], then the exact values k / w, (k + 0.5) / w, 0, 1, -1, +-1e-7 in u against the
    same kind in v (texel edges and centres of every period, both signs) and against random partners"""
    rng = np.random.default_rng([seed, h, w])
    u, v = rng.uniform(-3.0, 4.0, 3000), rng.uniform(-3.0, 4.0, 3000)

    def exact(n):
        k = np.arange(-3 * n, 4 * n + 1, dtype=np.float64)
        return np.concatenate([k / n, (k + 0.5) / n, [0.0, 1.0, -1.0, 1e-7, -1e-7]])

    eu, ev = exact(w), exact(h)
    n = max(len(eu), len(ev))
    eu, ev = np.resize(eu, n), np.resize(ev, n)
    u = np.concatenate([u, eu, eu, rng.uniform(-3.0, 4.0, n), rng.permutation(eu)])
    v = np.concatenate([v, ev, rng.uniform(-3.0, 4.0, n), ev, rng.permutation(ev)])
    return u.astype(np.float32), v.astype(np.float32)


@pytest.fixture(scope="module")
def readings():
    """per shape: the texture, the float32 uv and the two float32 readings at them (computed once)"""
    cpu = oa.OracleRenderer(8, 8)
    out = {}
    for k, (h, w) in enumerate(tx.SHAPES):
        tex = tx.random_texture(h, w)
        index = cpu.add_texture(tex)
        u, v = uv_samples(h, w, 41)
        orc = np.array([cpu.sample_texture(index, float(a), float(b)) for a, b in zip(u, v)], np.float32)
        ref = fw.sample_texture([tex], np.zeros(len(u), np.int64), u, v)
        out[(h, w)] = (tex, u, v, orc, ref)
    return out


def test_textures_have_distinct_texels():
    for h, w in tx.SHAPES:
        tex = tx.random_texture(h, w)
        assert len(np.unique(tex[..., :3].reshape(-1, 3), axis=0)) == h * w
        assert np.array_equal(tex, tx.random_texture(h, w)), "a fixed seed"


@pytest.mark.parametrize("shape", tx.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_readings_equal_each_other(readings, shape):
    tex, u, v, orc, ref = readings[shape]
    assert np.array_equal(orc.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("shape", tx.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_readings_stay_inside_the_envelope(readings, shape):
    tex, u, v, orc, ref = readings[shape]
    lo, hi = tx.envelope(tex, u, v, np.spacing(np.abs(u)).astype(np.float64), np.spacing(np.abs(v)).astype(np.float64))
    for name, got in (("oracle", orc), ("forward_reference", ref)):
        g = got.astype(np.float64)
        excess = np.maximum(lo - g, g - hi).max() / tx.ULP1
        use = tx.envelope_use(g, lo, hi, WIDEN).max()
        print(f"{shape} {name}: worst excess over the unwidened envelope {excess:.2f} ulp, use of the widened envelope {use:.3f}")
        assert (g >= lo - WIDEN).all() and (g <= hi + WIDEN).all(), (name, excess)


@pytest.mark.parametrize("shape", tx.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_reading_at_texel_centres_edges_and_mirrors(shape):
    """what the definition fixes without arithmetic: the texel itself at its centre, the mean of two neighbours on their common edge,
    the border texel on the texture's edge (the mirror image of itself), and the symmetries of MIRRORED_REPEAT"""
    h, w = shape
    tex = tx.random_texture(h, w)
    t = tex[..., :3].astype(np.float64) / 255.0
    ky, kx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cu, cv = ((kx + 0.5) / w).reshape(-1), ((ky + 0.5) / h).reshape(-1)
    assert np.abs(tx.sample(tex, cu, cv) - t.reshape(-1, 3)).max() < 1e-12
    for shift_u, shift_v in ((2, 0), (0, -2), (-2, 4)):  # the period is 2
        assert np.abs(tx.sample(tex, cu + shift_u, cv + shift_v) - t.reshape(-1, 3)).max() < 1e-12
    assert np.abs(tx.sample(tex, -cu, cv) - t.reshape(-1, 3)).max() < 1e-12, "u -> -u"
    assert np.abs(tx.sample(tex, cu, 2.0 - cv) - t.reshape(-1, 3)).max() < 1e-12, "v -> 2 - v"
    if w > 1:
        k = np.arange(1, w)
        edge = tx.sample(tex, k / w, np.full(len(k), 0.5 / h))
        assert np.abs(edge - 0.5 * (t[0, k - 1] + t[0, k])).max() < 1e-12
    for e in (0.0, 1.0, -1.0, 2.0):  # an edge of the texture: both texels of the footprint are the border texel
        col = 0 if e in (0.0, 2.0) else w - 1
        assert np.abs(tx.sample(tex, np.full(h, e), (np.arange(h) + 0.5) / h) - t[:, col]).max() < 1e-12
    i = np.arange(-4 * w, 4 * w)
    m = tx.mirrored_repeat(i, w)
    assert m.min() == 0 and m.max() == w - 1
    assert np.array_equal(m[4 * w:5 * w], np.arange(w)) and np.array_equal(m[5 * w:6 * w], np.arange(w)[::-1])
    assert np.array_equal(m[3 * w:4 * w], np.arange(w)[::-1]), "index -1 is texel 0"


def test_envelope_is_the_filters_range_over_the_box():
    """against brute force: a dense sampling of the box never leaves the envelope and comes close to both of its ends"""
    tex = tx.random_texture(3, 7)
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-3, 4, 40), rng.uniform(-3, 4, 40)
    du, dv = rng.uniform(0.0, 0.3, 40), rng.uniform(0.0, 0.5, 40)  # boxes over several cells
    lo, hi = tx.envelope(tex, u, v, du, dv)
    s = np.linspace(-1.0, 1.0, 61)
    gu, gv = np.meshgrid(s, s, indexing="ij")
    for k in range(40):
        f = tx.sample(tex, u[k] + du[k] * gu.reshape(-1), v[k] + dv[k] * gv.reshape(-1))
        assert (f >= lo[k] - 1e-12).all() and (f <= hi[k] + 1e-12).all()
        assert (f.min(0) - lo[k]).max() < 0.05 and (hi[k] - f.max(0)).max() < 0.05
    point = tx.envelope(tex, u, v, 0.0, 0.0)
    assert np.abs(point[0] - tx.sample(tex, u, v)).max() < 1e-15 and np.abs(point[1] - point[0]).max() < 1e-15

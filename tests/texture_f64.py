"""A float64 reading of the texture sampler (utopian/src/texture.rs:85-98: RGBA8 UNORM, LINEAR mag / min filter, MIRRORED_REPEAT in
both axes, level 0), written from the sampler's definition and from nothing in this repository: no tiling, no table, no float32.

  texel space   x = u * w - 0.5,  y = v * h - 0.5        (texel k's centre lies at u = (k + 0.5) / w)
  footprint     i = floor(x), i + 1;  j = floor(y), j + 1;  weights a = x - i, b = y - j
  addressing    MIRRORED_REPEAT as Vulkan states it: texel = (n - 1) - mirror((i mod 2n) - n), mirror(f) = f if f >= 0 else -(1 + f)
  value         c / 255 per channel, (1 - a)(1 - b) t00 + a (1 - b) t10 + (1 - a) b t01 + a b t11

The textures are row-major (h, w, 4) uint8 arrays; every function takes arrays of coordinates and returns float64.

envelope() is what a float32 sampler is held against: its input uv carries a rounding error, so its result can only be asked to lie
within the range the exact filter takes over a small box of uv around the nominal point. The filter is continuous and bilinear within
each cell of the texel-centre grid, so over a rectangle inside one cell its extrema lie at the rectangle's corners; a box that
straddles grid lines is cut along them, and the extrema lie at the corners of the pieces."""
import numpy as np

ULP1 = float(np.spacing(np.float32(1.0)))  # one float32 unit in the last place of 1.0

# What a float32 sampler may differ by from the exact filter's range over [u +- spacing(u)] x [v +- spacing(v)], in float32 ulp of 1.0.
# Reasoned: texel values and weights lie in [0, 1]; c / 255, 1 - a and the three lerps (two products and a sum each) round to half an ulp
# of values <= 1, and the products' errors are scaled by weights that sum to 1 - about 4 ulp for the chain. The texel-space
# coordinate u * w - 0.5 rounds twice: the product's half ulp is within spacing(u) * w, which the box covers; the difference's half
# ulp is at most that again where |u * w| > 0.5 (still inside a box of one spacing either side) and below 2^-25 texels nearer to 0,
# which times a texel difference <= 1 is a quarter ulp. Measured by test_texture_f64_cpu.py::test_float32_readings_stay_inside_the_envelope over all shapes:
# the worst excess of either reading over the unwidened envelope is 2.61 ulp (shape 9 x 17; 0.6 to 0.9 ulp on the others), so the 4 ulp
# hold without further widening.
WIDEN_ULP = 4
WIDEN = WIDEN_ULP * ULP1


def mirrored_repeat(i, n):
    """texel index in [0, n) of the unbounded index i (integer array) under MIRRORED_REPEAT"""
    f = np.mod(np.asarray(i, np.int64), 2 * n) - n  # numpy's mod takes the sign of the divisor: [0, 2n) - n
    return (n - 1) - np.where(f >= 0, f, -(1 + f))


def footprint(tex, u, v):
    """(i, j): the unbounded indices floor(x), floor(y) of the footprint's first texel; the footprint is (i, i + 1) x (j, j + 1)"""
    h, w = tex.shape[:2]
    x, y = np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5
    return np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)


def filter_texels(tex, x, y):
    """the bilinear filter at texel-space coordinates (x, y): (N, 3) float64"""
    h, w = tex.shape[:2]
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    fx, fy = np.floor(x), np.floor(y)
    a, b = (x - fx)[..., None], (y - fy)[..., None]
    i, j = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = mirrored_repeat(i, w), mirrored_repeat(i + 1, w), mirrored_repeat(j, h), mirrored_repeat(j + 1, h)
    t = tex[..., :3].astype(np.float64) / 255.0
    return (1.0 - a) * (1.0 - b) * t[y0, x0] + a * (1.0 - b) * t[y0, x1] + (1.0 - a) * b * t[y1, x0] + a * b * t[y1, x1]


def sample(tex, u, v):
    """the sampler at (u, v): (N, 3) float64"""
    h, w = tex.shape[:2]
    return filter_texels(tex, np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5)


def _cuts(lo, hi):
    """(K, N): per point the candidate coordinates of [lo, hi] - both ends, the middle and every integer in between (rows beyond
    a point's own count repeat its upper end)"""
    first = np.ceil(lo)
    count = np.maximum(np.floor(hi) - first + 1.0, 0.0)
    rows = [lo, 0.5 * (lo + hi), hi]
    for k in range(int(count.max()) if count.size else 0):
        rows.append(np.where(k < count, first + k, hi))
    return np.stack(rows)


def envelope(tex, u, v, du, dv):
    """(lo, hi), each (N, 3) float64: the per-channel range of the filter over the box [u - du, u + du] x [v - dv, v + dv] - its
    values at the box's corners and centre and, where the box holds lines of the texel-centre grid, on those lines too"""
    h, w = tex.shape[:2]
    u, v, du, dv = (np.atleast_1d(np.asarray(a, np.float64)) for a in (u, v, du, dv))
    du, dv = np.broadcast_to(du, u.shape), np.broadcast_to(dv, v.shape)
    xs = _cuts((u - du) * w - 0.5, (u + du) * w - 0.5)
    ys = _cuts((v - dv) * h - 0.5, (v + dv) * h - 0.5)
    lo = np.full(u.shape + (3,), np.inf)
    hi = np.full(u.shape + (3,), -np.inf)
    for x in xs:
        for y in ys:
            f = filter_texels(tex, x, y)
            lo, hi = np.minimum(lo, f), np.maximum(hi, f)
    return lo, hi


def envelope_use(value, lo, hi, widen):
    """how much of the envelope a result uses, per point: 0 on the envelope's middle, 1 on the edge of the envelope widened by
    `widen` on both sides, more than 1 outside it"""
    value = np.asarray(value, np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) + widen
    return (np.abs(value - mid) / half).max(axis=-1)


# ---- the textures of the tests: (h, w) as numpy has them ------------------------------------------------------------------------
ROW_MAJOR = [(1, 1), (1, 5), (7, 1), (2, 2), (3, 7), (9, 17), (12, 8), (8, 12)]  # a side that is no multiple of 8: rows as uploaded
TILED = [(8, 16), (16, 8), (8, 24), (24, 40)]                                    # 8 x 8 tiles, not square
SHAPES = ROW_MAJOR + TILED + [(8, 8)]                                            # and the square tile as a control


def random_texture(h, w, seed=0x7E7):
    """random bytes from a fixed seed; no two texels of a texture share their red, green and blue bytes, so a wrong address cannot
    read a right value"""
    rng = np.random.default_rng([seed, h, w])
    rgb = rng.choice(1 << 24, size=h * w, replace=False).astype(np.uint32)
    tex = np.empty((h, w, 4), np.uint8)
    for c in range(3):
        tex[..., c] = ((rgb >> (8 * c)) & 0xFF).reshape(h, w)
    tex[..., 3] = rng.integers(0, 256, (h, w))
    return tex

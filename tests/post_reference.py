"""The HDR display chain of the hybrid frame (UH_HYBRID_POST, uh_post_image) restated in numpy: DESIGN.md section 2, "HDR display chain:
the arithmetic contract of UH_HYBRID_POST", operation for operation in float32 - the histogram, the exposure with its integer
arithmetic, the prefilter, the down and up filters, the composite with its three operators and the bad-pixel rule. The device is held
to it bit for bit (tests/test_gpu_post.py). Every image function takes the number format, so the same formulas evaluate in float64 too
(`evaluate` with dtype=np.float64): what tests/test_post_cpu.py measures the float32 rounding against.

max(a, b) is `a if a > b else b` and min likewise, as in the contract: the sign of a zero result is then defined."""
import numpy as np

F = np.float32
MAX_SAMPLE = F(2.0 ** 48)  # temporal_sample_ok's bound
AUTO_EXPOSURE, BLOOM = 1, 2
NONE, REINHARD, ACES = 0, 1, 2
BINS = 256
MAX_LEVELS = 8
SIZES = [(1, 1), (1, 45), (67, 1), (65, 3), (257, 3), (97, 61)]  # (W, H): the hybrid size list
DEFAULTS = dict(flags=AUTO_EXPOSURE | BLOOM, tonemap=ACES, bloom_levels=6, manual_exposure=1.0, key=0.18, min_exposure=0.015625,
                max_exposure=64.0, adaptation=0.1, low_percentile=0.5, high_percentile=0.95, bloom_threshold=1.0, bloom_intensity=0.04)
_FLOATS = [k for k, v in DEFAULTS.items() if isinstance(v, float)]


def params(**fields):
    """the defaults of uh_post_default_params with `fields` replaced; the float fields as float32"""
    p = dict(DEFAULTS, **fields)
    assert set(p) == set(DEFAULTS), set(p) - set(DEFAULTS)
    for k in _FLOATS:
        p[k] = F(p[k])
    return p


def params_of(c):
    """a PostParams structure as the dictionary above"""
    return params(**{k: getattr(c, k) for k in DEFAULTS})


def pmax(a, b):
    return np.where(a > b, a, b)


def pmin(a, b):
    return np.where(a < b, a, b)


def luminance(rgb):
    """dn_luminance: (0.299 r + 0.587 g) + 0.114 b"""
    t = rgb.dtype.type
    return (t(F(0.299)) * rgb[..., 0] + t(F(0.587)) * rgb[..., 1]) + t(F(0.114)) * rgb[..., 2]


def bad_mask(img):
    """pixels that fail temporal_sample_ok: a colour channel NaN, infinite or above 2^48 in magnitude"""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(img[..., :3]) <= MAX_SAMPLE).all(axis=-1)


# ---- level sizes ----------------------------------------------------------------------------------------------------------------------
def level_size(W, H, level):
    """(w, h) of `level` (0: the frame), None when it does not exist"""
    if W < 1 or H < 1 or level > MAX_LEVELS:
        return None
    for _ in range(level):
        if (W, H) == (1, 1):
            return None
        W, H = (W + 1) // 2, (H + 1) // 2
    return W, H


def level_count(W, H, bloom_levels):
    n = 0
    while n < min(bloom_levels, MAX_LEVELS) and level_size(W, H, n + 1) is not None:
        n += 1
    return n


# ---- metering -------------------------------------------------------------------------------------------------------------------------
def histogram(img):
    """the 256 counts of an (H, W, 4) float32 image: bin = clamp((bits(L) >> 20) - 888, 0, 255); L <= 0, NaN and bad pixels in bin 0"""
    img = np.asarray(img, F)
    with np.errstate(all="ignore"):
        L = luminance(img[..., :3]).astype(F)
        ok = ~bad_mask(img) & (L > 0)
    b = np.clip((np.ascontiguousarray(L).view(np.uint32) >> 20).astype(np.int64) - 888, 0, BINS - 1)
    return np.bincount(np.where(ok, b, 0).reshape(-1), minlength=BINS).astype(np.uint32)


def metered_average(hist, low, high):
    """(Lavg, n): the float whose bits are the mean bin of the samples ranked [lo, hi) through the inverse map, and the metered count;
    Lavg is None when nothing is metered"""
    counts = [int(c) for c in hist]
    counts[0] = 0
    n = sum(counts)
    lo, hi = int(float(F(low)) * n), int(float(F(high)) * n)
    Sb = N = begin = 0
    for b, m in enumerate(counts):
        end = begin + m
        kept = max(0, min(end, hi) - max(begin, lo)) if hi > lo else m
        Sb, N, begin = Sb + kept * b, N + kept, end
    if N == 0:
        return None, n
    q = (888 << 20) + ((Sb << 20) // N) + (1 << 19)
    return np.array([q], np.uint32).view(F)[0], n


def exposure(hist, p, prev):
    """the exposure record of one pass: hist None without AUTO_EXPOSURE; prev the previous pass's E or None. (E, target, Lavg, n)"""
    if hist is None:
        return p["manual_exposure"], p["manual_exposure"], F(0), 0
    lavg, n = metered_average(hist, p["low_percentile"], p["high_percentile"])
    if lavg is None:
        E = p["manual_exposure"] if prev is None else F(prev)
        return E, E, F(0), n
    target = F(pmin(pmax(p["key"] / lavg, p["min_exposure"]), p["max_exposure"]))
    E = target if prev is None else F(F(prev) + F(F(target - F(prev)) * p["adaptation"]))
    return E, target, lavg, n


# ---- bloom ----------------------------------------------------------------------------------------------------------------------------
def prefilter(img, E, threshold, dtype=F):
    """(H, W, 3): 0 for a bad pixel and unless the largest exposed channel m > threshold, else c ((m - threshold) / m)"""
    t = dtype
    with np.errstate(all="ignore"):
        c = np.asarray(img)[..., :3].astype(t) * t(E)
        m = pmax(pmax(c[..., 0], c[..., 1]), c[..., 2])
        f = (m - t(threshold)) / m
        keep = ~bad_mask(np.asarray(img, F)) & (m > t(threshold))
        return np.where(keep[..., None], c * f[..., None], t(0)).astype(t)


def down(src):
    """one level down: taps (1, 3, 3, 1) / 8 per axis at 2X - 1 .. 2X + 2, clamped; acc = acc + weight * texel, rows outer, columns inner"""
    t = src.dtype.type
    h, w = src.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    X, Y = np.arange(dw), np.arange(dh)
    acc = np.zeros((dh, dw, 3), t)
    for j in range(4):
        sy = np.clip(2 * Y - 1 + j, 0, h - 1)
        for i in range(4):
            sx = np.clip(2 * X - 1 + i, 0, w - 1)
            weight = t((1 if i in (0, 3) else 3) * (1 if j in (0, 3) else 3)) * t(0.015625)
            acc = acc + weight * src[sy][:, sx]
    return acc


def upsample(img, w, h):
    """U(img) into w x h: even x takes x/2 - 1 at 0.25 and x/2 at 0.75, odd x (x-1)/2 at 0.75 and (x+1)/2 at 0.25, clamped; y the same"""
    t = img.dtype.type
    sh, sw = img.shape[:2]

    def taps(n, sn):
        x = np.arange(n)
        odd = (x & 1) == 1
        a = np.clip(np.where(odd, (x - 1) // 2, x // 2 - 1), 0, sn - 1)
        b = np.clip(np.where(odd, (x + 1) // 2, x // 2), 0, sn - 1)
        return a, b, np.where(odd, t(0.75), t(0.25)).astype(t), np.where(odd, t(0.25), t(0.75)).astype(t)

    x0, x1, wx0, wx1 = taps(w, sw)
    y0, y1, wy0, wy1 = taps(h, sh)
    acc = np.zeros((h, w, 3), t)
    for ys, wy, xs, wx in ((y0, wy0, x0, wx0), (y0, wy0, x1, wx1), (y1, wy1, x0, wx0), (y1, wy1, x1, wx1)):
        acc = acc + (wx[None, :] * wy[:, None])[..., None] * img[ys][:, xs]
    return acc


def bloom(img, E, p, dtype=F):
    """(down, up): dictionaries level -> (h, w, 3) image, empty without a level"""
    H, W = np.asarray(img).shape[:2]
    n = level_count(W, H, p["bloom_levels"])
    dn, up = {}, {}
    src = prefilter(img, E, p["bloom_threshold"], dtype)
    for k in range(1, n + 1):
        src = dn[k] = down(src)
    for k in range(n, 0, -1):
        up[k] = dn[k] if k == n else (dn[k] + upsample(up[k + 1], dn[k].shape[1], dn[k].shape[0])) * dtype(0.5)
    return dn, up


# ---- composite ------------------------------------------------------------------------------------------------------------------------
def tonemap(x, op):
    t = x.dtype.type
    if op == NONE:
        return x
    xc = pmin(pmax(x, t(0)), t(1048576))
    if op == REINHARD:
        return xc / (xc + t(1))
    a = xc * (t(F(2.51)) * xc + t(F(0.03)))
    b = xc * (t(F(2.43)) * xc + t(F(0.59))) + t(F(0.14))
    return pmin(pmax(a / b, t(0)), t(1))


def composite(img, E, up1, p, dtype=F):
    """post_output (H, W, 4) float32: the operator over S.rgb E + bloom_intensity U(up[1]); a bad pixel is its S texel, bits unchanged"""
    img = np.ascontiguousarray(img, F)
    H, W = img.shape[:2]
    with np.errstate(all="ignore"):
        x = img[..., :3].astype(dtype) * dtype(E)
        if up1 is not None:
            x = x + dtype(p["bloom_intensity"]) * upsample(up1, W, H)
        y = tonemap(x, p["tonemap"]).astype(F)
    out = img.copy()
    ob, yb = out.view(np.uint32), np.ascontiguousarray(y).view(np.uint32)
    good = ~bad_mask(img)
    ob[..., :3][good] = yb[good]
    return out


def evaluate(img, p, E, dtype=F):
    """bloom and composite of one image at exposure E in `dtype`: dict(output, down, up)"""
    dn, up = bloom(img, E, p, dtype) if p["flags"] & BLOOM else ({}, {})
    return dict(output=composite(img, E, up.get(1), p, dtype), down=dn, up=up)


class Post:
    """the chain with its exposure state: call it per pass with the source image and the params; reset() is uh_reset_post_exposure"""

    def __init__(self):
        self.E = None

    def reset(self):
        self.E = None

    def __call__(self, img, p):
        img = np.ascontiguousarray(img, F)
        hist = histogram(img) if p["flags"] & AUTO_EXPOSURE else None
        E, target, lavg, n = exposure(hist, p, self.E)
        self.E = E
        r = evaluate(img, p, E)
        r.update(histogram=hist, exposure=F(E), target=F(target), lavg=F(lavg), metered=n, bad=int(bad_mask(img).sum()), levels=len(r["down"]))
        return r

"""UH_HYBRID_TAA restated in numpy, from DESIGN.md section 2 "Temporal anti-aliasing: the arithmetic contract of UH_HYBRID_TAA": every
operation float32, in the order written there. Not a test module: test_taa_cpu.py holds it to known answers, test_gpu_taa.py holds the
device to it on the device's own read-backs."""
import numpy as np

F = np.float32
CLAMP, MOTION = 1, 2
MAX_SAMPLE = F(2.0 ** 48)  # the largest channel magnitude of a colour that takes part ("Non-finite input")


def sample_ok(c):
    """every channel of c (..., 3) finite and at most MAX_SAMPLE in magnitude; a NaN fails the compare"""
    with np.errstate(all="ignore"):
        return (np.abs(c) <= MAX_SAMPLE).all(axis=-1)


def default_params(**kw):
    p = dict(flags=CLAMP, max_history=16, alpha_min=0.1, clamp_gamma=1.0)
    p.update(kw)
    return p


def params_of(p):
    """the same dict from a TaaParams structure"""
    return {k: getattr(p, k) for k in default_params()}


def mat4_mul(m, x, y, z, w):
    """column-major mat4 * vec4: ((c0 x + c1 y) + c2 z) + c3 w, the four rows"""
    return [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w for r in range(4)]


def primary_directions(view, W, H):
    """the direction of primary_ray(x, y, 0.5, 0.5) for every pixel, (H * W, 3) float32 ("primary rays")"""
    iv, ip = np.array(view.inverse_view[:], np.float32), np.array(view.inverse_projection[:], np.float32)
    y, x = np.mgrid[0:H, 0:W]
    cx, cy = x.reshape(-1).astype(np.float32) + F(0.5), y.reshape(-1).astype(np.float32) + F(0.5)
    u, v = cx / F(W), cy / F(H)
    v = F(1.0) - v
    dx, dy = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    one = np.ones_like(dx)
    tg = mat4_mul(ip, dx, dy, one, one)
    inv = F(1.0) / np.sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2])
    nt = [tg[0] * inv, tg[1] * inv, tg[2] * inv]
    d = mat4_mul(iv, nt[0], nt[1], nt[2], np.zeros_like(dx))
    return np.stack(d[:3], axis=-1)


def box(c, W, H, gamma):
    """(lo, hi) of step 1 for every pixel: c (H * W, 3) float32. Neighbours that are not sample_ok are left out like those outside the
    frame; the box of a pixel that is itself not sample_ok is never read (k may be 0 there)"""
    img = c.reshape(H, W, 3)
    live = sample_ok(img)
    s1, s2, k = np.zeros_like(img), np.zeros_like(img), np.zeros((H, W, 1), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qx, qy = x + dx, y + dy
            inside = ((qx >= 0) & (qx < W) & (qy >= 0) & (qy < H))[..., None]
            q = img[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            inside = inside & live[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)][..., None]
            s1 = np.where(inside, s1 + q, s1)
            s2 = np.where(inside, s2 + q * q, s2)
            k = np.where(inside, k + F(1.0), k)
    m1, m2 = s1 / k, s2 / k
    sg = np.sqrt(np.maximum(m2 - m1 * m1, F(0.0)))
    g = F(gamma)
    return (m1 - g * sg).reshape(-1, 3), (m1 + g * sg).reshape(-1, 3)


class Taa:
    """one context's resolve: call() is the taa pass of uh_render_hybrid, reset() is uh_reset_taa_history"""

    def __init__(self):
        self.hist = None

    def reset(self):
        self.hist = None

    def __call__(self, deferred, position, motion, view, params, W, H):
        """deferred, position (H, W, 4) float32, motion (H, W, 4) float32 or None (required with the MOTION flag), view a ViewUniformData
        (or anything with inverse_view, inverse_projection and prev_frame_projection_view), params a dict as default_params(). Returns
        dict(output (H, W, 4), history (H, W), blended, bad (H, W) bool, history_pixels, reset_pixels, lo, hi (H, W, 3) or None)."""
        p = params
        flags = int(p["flags"])
        with np.errstate(all="ignore"):
            c4 = np.ascontiguousarray(deferred, np.float32).reshape(-1, 4)
            c = c4[:, :3]
            n = len(c)
            lo = hi = None
            if flags & CLAMP:
                lo, hi = box(c, W, H, p["clamp_gamma"])
            live = sample_ok(c)
            out, N = c.copy(), np.where(live, F(1.0), F(0.0))
            blended = np.zeros(n, bool)
            if self.hist is not None:
                pv = np.array(view.prev_frame_projection_view[:], np.float32)
                P4 = position.reshape(-1, 4)
                geo = P4[:, 3] != 0
                Q = P4[:, :3]
                corresponds = np.ones(n, bool)
                if flags & MOTION:
                    m4 = motion.reshape(-1, 4)
                    Q = np.where(geo[:, None], m4[:, :3], Q)
                    corresponds = np.where(geo, m4[:, 3] != 0, True)
                d = primary_directions(view, W, H)
                one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
                hg = mat4_mul(pv, Q[:, 0], Q[:, 1], Q[:, 2], one)
                hs = mat4_mul(pv, d[:, 0], d[:, 1], d[:, 2], zero)
                h = [np.where(geo, a, b) for a, b in zip(hg, hs)]
                u = (h[0] / h[3]) * F(0.5) + F(0.5)
                v = F(1.0) - ((h[1] / h[3]) * F(0.5) + F(0.5))
                fx, fy = u * F(W) - F(0.5), v * F(H) - F(0.5)
                ok = live & corresponds & (h[3] > 0) & np.isfinite(fx) & np.isfinite(fy)
                fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
                ix, iy = np.floor(fx), np.floor(fy)
                ax, ay = np.rint((fx - ix) * F(256.0)) / F(256.0), np.rint((fy - iy) * F(256.0)) / F(256.0)
                sw = np.zeros(n, np.float32)
                sums = [np.zeros(n, np.float32) for _ in range(4)]  # r, g, b, N
                pc, pn = self.hist
                self.taps = []  # (in the frame with a weight, index, weight) of the four taps, for tests that reason about them
                for t in range(4):
                    dx, dy = t & 1, t >> 1
                    w = (ax if dx else F(1.0) - ax) * (ay if dy else F(1.0) - ay)
                    tx, ty = ix + F(dx), iy + F(dy)
                    valid = ok & (w != 0) & (tx >= 0) & (tx <= F(W - 1)) & (ty >= 0) & (ty <= F(H - 1))
                    j = np.where(valid, ty, F(0.0)).astype(np.int64) * W + np.where(valid, tx, F(0.0)).astype(np.int64)
                    self.taps.append((valid.copy(), j, w))
                    valid &= pn[j] != 0  # a texel that was not sample_ok left no history
                    sw = np.where(valid, sw + w, sw)
                    taps = [pc[j, 0], pc[j, 1], pc[j, 2], pn[j]]
                    sums = [np.where(valid, s + w * q, s) for s, q in zip(sums, taps)]
                blended = sw > 0
                swd = np.where(blended, sw, F(1.0))
                Nn = np.minimum(sums[3] / swd + F(1.0), F(int(p["max_history"])))
                a = np.maximum(F(1.0) / Nn, F(p["alpha_min"]))
                hc = np.stack([sums[k] / swd for k in range(3)], axis=-1)
                if flags & CLAMP:
                    # no NaN reaches the clamp: hc is a mean of history values, which are finite, and lo, hi come from neighbours that are
                    # sample_ok (gamma * sg may overflow to +Inf, which only opens the box); fminf / fmaxf and these agree on such values
                    assert not (np.isnan(hc[blended]).any() or np.isnan(lo[blended]).any() or np.isnan(hi[blended]).any())
                    hc = np.minimum(np.maximum(hc, lo), hi)
                mixed = hc + (c - hc) * a[:, None]
                out = np.where(blended[:, None], mixed, c)
                N = np.where(blended, Nn, np.where(live, F(1.0), F(0.0)))
            self.hist = (out.copy(), N.copy())
        output = np.concatenate([out, c4[:, 3:4]], axis=-1).reshape(H, W, 4)
        shaped = lambda a: None if a is None else a.reshape(H, W, 3)
        return dict(output=output, history=N.reshape(H, W), blended=blended.reshape(H, W), bad=~live.reshape(H, W), history_pixels=int(blended.sum()),
                    reset_pixels=int(n - blended.sum()), lo=shaped(lo), hi=shaped(hi))

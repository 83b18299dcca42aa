"""uh_denoise restated in numpy, from DESIGN.md section 2 "Denoiser: the arithmetic contract of uh_denoise": every operation float32, in
the order written there; numpy.exp stands where the device calls expf. Not a test module: test_denoise_cpu.py holds it to known answers,
test_gpu_denoise.py holds the device to it on the device's own read-backs."""
import numpy as np

F = np.float32
TEMPORAL, DEMODULATE = 1, 2
KERNEL = {0: F(0.375), 1: F(0.25), 2: F(0.0625)}
CENTRE = F(0.140625)  # 9/64
MAX_SAMPLE = F(2.0 ** 48)  # the largest channel magnitude of a sample that takes part ("Non-finite input")


def sample_ok(c):
    """every channel of c (..., 3) finite and at most MAX_SAMPLE in magnitude; a NaN fails the compare"""
    with np.errstate(all="ignore"):
        return (np.abs(c) <= MAX_SAMPLE).all(axis=-1)


def live_geometry(position, acc, n):
    """(drawn, live): the pixels the G-buffer wrote (position w != 0), and those of them whose stage-0 colour acc / n, before
    demodulation, is a sample the filter takes in. A drawn pixel that is not live is treated as not geometry everywhere"""
    drawn = position.reshape(-1, 4)[:, 3] != 0
    with np.errstate(all="ignore"):
        return drawn, drawn & sample_ok(acc.reshape(-1, 4)[:, :3] / n)


def default_params(**kw):
    p = dict(flags=TEMPORAL | DEMODULATE, iterations=5, max_history=32, alpha_min=0.2, sigma_luminance=4.0, sigma_plane=0.005,
             reproject_normal_cos=0.9, reproject_plane=0.005)
    p.update(kw)
    return p


def params_of(p):
    """the same dict from a DenoiseParams structure"""
    return {k: getattr(p, k) for k in default_params()}


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def luminance(c):
    return (F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2]


def linear_to_srgb(c):
    """view.glsl:53-61 with pow in double, rounded to float"""
    with np.errstate(all="ignore"):
        p = np.power(c.astype(np.float64), np.float64(F(1.0) / F(2.4))).astype(np.float32)
        return np.where(c < F(0.0031308), c * F(12.92), F(1.055) * p - F(0.055))


def unorm8(x):
    x = np.where(x > 0, x, F(0.0))
    x = np.where(x > 1, F(1.0), x)
    return np.rint(x * F(255.0)).astype(np.uint8)


def normal_weight(a, b):
    t = np.maximum(dot3(a, b), F(0.0))
    for _ in range(7):
        t = t * t
    return t


def _shift(H, W, dx, dy):
    """flat indices of pixel (x + dx, y + dy) for every pixel, clipped, and whether it lies inside the image"""
    y, x = np.mgrid[0:H, 0:W]
    qx, qy = x + dx, y + dy
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    return (np.clip(qy, 0, H - 1) * W + np.clip(qx, 0, W - 1)).reshape(-1), inside.reshape(-1)


class Denoiser:
    """one context's denoiser: call() is uh_denoise, reset() is uh_reset_denoise_history"""

    def __init__(self):
        self.hist = None

    def reset(self):
        self.hist = None

    def __call__(self, acc, position, normal, albedo, pbr, view, params):
        """acc, position, normal, pbr (H, W, 4) float32, albedo (H, W, 4) uint8, view a ViewUniformData (or anything with its fields),
        params a dict as default_params(). Returns the six images of uh_read_denoised by name, `kept`, `geometry` (position w != 0: what
        UhDenoiseStats.geometry_pixels counts) and `bad` (geometry the filter treated as not geometry) (H, W) bool."""
        p = params
        H, W = acc.shape[:2]
        n = F(min(int(view.total_samples), int(view.accumulation_limit)))
        vm = np.array(view.view[:], np.float32)
        pv = np.array(view.prev_frame_projection_view[:], np.float32)
        with np.errstate(all="ignore"):
            acc = acc.reshape(-1, 4)
            P = position.reshape(-1, 4)[:, :3]
            drawn, geo = live_geometry(position, acc, n)
            nrm = normal.reshape(-1, 4)[:, :3]
            mesh = pbr.reshape(-1, 4)[:, 3]
            # stage 0
            c = acc[:, :3] / n
            dm = np.ones_like(c)
            if p["flags"] & DEMODULATE:
                dm = np.where(geo[:, None], np.maximum(albedo.reshape(-1, 4)[:, :3].astype(np.float32) / F(255.0), F(0.01)), F(1.0))
                c = np.where(geo[:, None], c / dm, c)
            inp = c.copy()
            l = luminance(c)
            l2 = l * l
            z = ((vm[2] * P[:, 0] + vm[6] * P[:, 1]) + vm[10] * P[:, 2]) + vm[14] * F(1.0)
            # stage 1
            col, m1, m2, N = c.copy(), l.copy(), l2.copy(), np.ones(len(c), np.float32)
            kept = np.zeros(len(c), bool)
            if (p["flags"] & TEMPORAL) and self.hist is not None:
                hp = self.hist
                h = [((pv[r] * P[:, 0] + pv[4 + r] * P[:, 1]) + pv[8 + r] * P[:, 2]) + pv[12 + r] * F(1.0) for r in range(4)]
                u = (h[0] / h[3]) * F(0.5) + F(0.5)
                v = F(1.0) - ((h[1] / h[3]) * F(0.5) + F(0.5))
                fx, fy = u * F(W) - F(0.5), v * F(H) - F(0.5)
                ok = geo & (h[3] > 0) & np.isfinite(fx) & np.isfinite(fy)
                fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
                ix, iy = np.floor(fx), np.floor(fy)
                ax, ay = np.rint((fx - ix) * F(256.0)) / F(256.0), np.rint((fy - iy) * F(256.0)) / F(256.0)
                tol = F(p["reproject_plane"]) * np.abs(z)
                sw = np.zeros(len(c), np.float32)
                sums = [np.zeros(len(c), np.float32) for _ in range(6)]  # r, g, b, N, m1, m2
                self.taps = []  # (in the frame with a weight, index, weight) of the four taps, for tests that reason about them
                for t in range(4):
                    dx, dy = t & 1, t >> 1
                    w = (ax if dx else F(1.0) - ax) * (ay if dy else F(1.0) - ay)
                    tx, ty = ix + F(dx), iy + F(dy)
                    valid = ok & (w != 0) & (tx >= 0) & (tx <= F(W - 1)) & (ty >= 0) & (ty <= F(H - 1))
                    j = np.where(valid, ty, F(0.0)).astype(np.int64) * W + np.where(valid, tx, F(0.0)).astype(np.int64)
                    self.taps.append((valid.copy(), j, w))
                    valid &= hp["geo"][j]
                    valid &= hp["mesh"][j] == mesh
                    valid &= dot3(nrm, hp["nrm"][j]) >= F(p["reproject_normal_cos"])
                    valid &= np.abs(dot3(hp["pos"][j] - P, nrm)) <= tol
                    sw = np.where(valid, sw + w, sw)
                    taps = [hp["col"][j, 0], hp["col"][j, 1], hp["col"][j, 2], hp["N"][j], hp["m1"][j], hp["m2"][j]]
                    sums = [np.where(valid, s + w * q, s) for s, q in zip(sums, taps)]
                kept = sw > 0
                swd = np.where(kept, sw, F(1.0))
                Nn = np.minimum(sums[3] / swd + F(1.0), F(p["max_history"]))
                al = np.maximum(F(1.0) / Nn, F(p["alpha_min"]))
                blend = lambda prev, x: prev + (x - prev) * al
                col = np.where(kept[:, None], np.stack([blend(sums[k] / swd, c[:, k]) for k in range(3)], axis=-1), c)
                m1 = np.where(kept, blend(sums[4] / swd, l), l)
                m2 = np.where(kept, blend(sums[5] / swd, l2), l2)
                N = np.where(kept, Nn, F(1.0))
            var = np.maximum(m2 - m1 * m1, F(0.0))
            col = np.where(geo[:, None], col, c)
            N = np.where(geo, N, F(0.0))
            var = np.where(geo, var, F(0.0))
            self.hist = dict(geo=geo.copy(), pos=P.copy(), nrm=nrm.copy(), mesh=mesh.copy(), col=col.copy(), N=N.copy(), m1=m1.copy(), m2=m2.copy())
            temporal = col * dm
            # stage 2
            plane_den = F(p["sigma_plane"]) * np.abs(z) + F(1e-6)
            short = geo & (N < 4)
            if short.any():
                sw, s1, s2 = (np.zeros(len(c), np.float32) for _ in range(3))
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        j, inside = _shift(H, W, dx, dy)
                        valid = inside & geo[j]
                        w = normal_weight(nrm, nrm[j]) * np.exp(-(np.abs(dot3(P[j] - P, nrm)) / plane_den))
                        sw = np.where(valid, sw + w, sw)
                        s1 = np.where(valid, s1 + w * m1[j], s1)
                        s2 = np.where(valid, s2 + w * m2[j], s2)
                swd = np.where(sw > 0, sw, F(1.0))
                a, b = s1 / swd, s2 / swd
                est = np.maximum(b - a * a, F(0.0)) * (F(4.0) / np.where(short, N, F(1.0)))
                var = np.where(short & (sw > 0), est, var)
            var0 = var.copy()
            # stage 3
            for level in range(int(p["iterations"])):
                s = 1 << level
                sg, sk = np.zeros(len(c), np.float32), np.zeros(len(c), np.float32)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        j, inside = _shift(H, W, dx, dy)
                        valid = inside & geo[j]
                        k = (F(0.5) if dx == 0 else F(0.25)) * (F(0.5) if dy == 0 else F(0.25))
                        sg = np.where(valid, sg + k * var[j], sg)
                        sk = np.where(valid, sk + k, sk)
                lum_den = F(p["sigma_luminance"]) * np.sqrt(sg / np.where(sk > 0, sk, F(1.0))) + F(1e-6)
                lp = luminance(col)
                sw = np.full(len(c), CENTRE, np.float32)
                sc = CENTRE * col
                sv = (CENTRE * CENTRE) * var
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        if dx == 0 and dy == 0:
                            continue
                        j, inside = _shift(H, W, s * dx, s * dy)
                        valid = inside & geo[j]
                        k = KERNEL[abs(dx)] * KERNEL[abs(dy)]
                        ep = np.abs(dot3(P[j] - P, nrm)) / plane_den
                        el = np.abs(lp - lp[j]) / lum_den
                        w = (k * normal_weight(nrm, nrm[j])) * np.exp(-(ep + el))
                        sw = np.where(valid, sw + w, sw)
                        sc = np.where(valid[:, None], sc + w[:, None] * col[j], sc)
                        sv = np.where(valid, sv + (w * w) * var[j], sv)
                col = np.where(geo[:, None], sc / sw[:, None], col)
                var = np.where(geo, sv / (sw * sw), var)
            # stage 4
            out = col * dm
            srgb = unorm8(linear_to_srgb(out))
        rgba = lambda a: np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=-1).reshape(H, W, 4)
        bgra = np.stack([srgb[:, 2], srgb[:, 1], srgb[:, 0], np.zeros(len(srgb), np.uint8)], axis=-1).reshape(H, W, 4)
        return dict(color=rgba(out), output=bgra, input=rgba(inp), temporal=rgba(temporal), history=N.reshape(H, W), variance=var0.reshape(H, W),
                    final_variance=var.reshape(H, W), kept=kept.reshape(H, W), geometry=drawn.reshape(H, W), bad=(drawn & ~geo).reshape(H, W))

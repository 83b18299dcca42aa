"""uh_denoise with UH_DENOISE_MOTION restated in numpy, from DESIGN.md section 2 "Motion vectors" (the denoiser's part): float32, in the
order written there. A geometry pixel whose motion texel has w != 0 reprojects the texel's xyz through prev_frame_projection_view and
holds the history taps' plane distance against it; one whose texel has w == 0 keeps no history. The tolerance (from the CURRENT view
depth), the normal and mesh tests, the weights and the blend are denoise_reference's. Its Denoiser is one function from the input to
the output, so the stages behind the temporal one are written out here as well, with its helpers; without the flag (or without a
temporal stage) the call is the base class's. Not a test module."""
import numpy as np

import denoise_reference as dr
from denoise_reference import CENTRE, KERNEL, F, _shift, dot3, linear_to_srgb, luminance, normal_weight, unorm8

MOTION = 8


def params_of(p):
    return dr.params_of(p)


class MotionDenoiser(dr.Denoiser):
    """call(acc, position, normal, albedo, pbr, motion, view, params): params["flags"] may carry MOTION"""

    def __call__(self, acc, position, normal, albedo, pbr, motion, view, params):
        p = dict(params)
        flags = int(p["flags"])
        p["flags"] = flags & ~MOTION
        if not (flags & MOTION) or not (flags & dr.TEMPORAL) or self.hist is None:
            return super().__call__(acc, position, normal, albedo, pbr, view, p)
        H, W = acc.shape[:2]
        n = F(min(int(view.total_samples), int(view.accumulation_limit)))
        vm = np.array(view.view[:], np.float32)
        pv = np.array(view.prev_frame_projection_view[:], np.float32)
        with np.errstate(all="ignore"):
            acc = acc.reshape(-1, 4)
            P = position.reshape(-1, 4)[:, :3]
            drawn, geo = dr.live_geometry(position, acc, n)
            PP = motion.reshape(-1, 4)[:, :3]                 # where the surface point was at the previous motion pass
            corresponds = motion.reshape(-1, 4)[:, 3] != 0
            nrm = normal.reshape(-1, 4)[:, :3]
            mesh = pbr.reshape(-1, 4)[:, 3]
            # stage 0
            c = acc[:, :3] / n
            dm = np.ones_like(c)
            if p["flags"] & dr.DEMODULATE:
                dm = np.where(geo[:, None], np.maximum(albedo.reshape(-1, 4)[:, :3].astype(np.float32) / F(255.0), F(0.01)), F(1.0))
                c = np.where(geo[:, None], c / dm, c)
            inp = c.copy()
            l = luminance(c)
            l2 = l * l
            z = ((vm[2] * P[:, 0] + vm[6] * P[:, 1]) + vm[10] * P[:, 2]) + vm[14] * F(1.0)  # the CURRENT view depth
            # stage 1: PP in the projection and in the plane test, nowhere else
            hp = self.hist
            h = [((pv[r] * PP[:, 0] + pv[4 + r] * PP[:, 1]) + pv[8 + r] * PP[:, 2]) + pv[12 + r] * F(1.0) for r in range(4)]
            u = (h[0] / h[3]) * F(0.5) + F(0.5)
            v = F(1.0) - ((h[1] / h[3]) * F(0.5) + F(0.5))
            fx, fy = u * F(W) - F(0.5), v * F(H) - F(0.5)
            ok = geo & corresponds & (h[3] > 0) & np.isfinite(fx) & np.isfinite(fy)
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
                valid &= np.abs(dot3(hp["pos"][j] - PP, nrm)) <= tol
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
            # stages 2 to 4: denoise_reference's, on the current position
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
            out = col * dm
            srgb = unorm8(linear_to_srgb(out))
        rgba = lambda a: np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=-1).reshape(H, W, 4)
        bgra = np.stack([srgb[:, 2], srgb[:, 1], srgb[:, 0], np.zeros(len(srgb), np.uint8)], axis=-1).reshape(H, W, 4)
        return dict(color=rgba(out), output=bgra, input=rgba(inp), temporal=rgba(temporal), history=N.reshape(H, W), variance=var0.reshape(H, W),
                    final_variance=var.reshape(H, W), kept=kept.reshape(H, W), geometry=drawn.reshape(H, W), bad=(drawn & ~geo).reshape(H, W))

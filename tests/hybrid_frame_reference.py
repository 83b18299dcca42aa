"""CPU reference of the hybrid graph's final frame (uh_render_hybrid's UH_HYBRID_SSAO / DEFERRED / SKY / PRESENT): ssao.frag,
deferred.frag + pbr_lighting.glsl / brdf.glsl, atmosphere.frag (cubemap off) and present.frag + fxaa.glsl, in numpy float32 in the order
DESIGN.md section 2 "Hybrid frame passes" pins, line by line. Built on tests/hybrid_reference.py and the oracle's primary_ray and sky.
Each pass takes its input images as arguments, so a test can feed it the device's own inputs. Not a conftest: test modules import it."""
import numpy as np

import hybrid_reference as hr
import oracle_api as oa

F = np.float32
PI = F(3.14159265359)  # brdf.glsl:1

# ssao.frag:31-64
SSAO_KERNEL = np.array([
    (-0.68217, 0.23565, 0.48243), (-0.14448, 0.01628, 0.22807), (0.00604, 0.01909, 0.0127), (0.09733, 0.39072, 0.7324),
    (0.06055, 0.87847, 0.33303), (0.00734, 0.19034, 0.13091), (-0.01377, 0.01745, 0.00399), (0.01468, 0.16627, 0.09108),
    (-0.10093, -0.08015, 0.06625), (-0.27125, -0.39937, 0.0601), (-0.06181, -0.03065, 0.01213), (-0.40189, -0.48095, 0.21808),
    (0.04027, -0.05818, 0.26542), (-0.33535, -0.07516, 0.24997), (0.32748, -0.18112, 0.27292), (0.53962, -0.03361, 0.58926),
    (-0.09598, -0.25424, 0.35754), (-0.17368, 0.01261, 0.23964), (0.1283, 0.12573, 0.16467), (-0.34418, 0.19403, 0.70285),
    (-0.09686, -0.0928, 0.11447), (0.32727, -0.49713, 0.17518), (0.12345, 0.13862, 0.23822), (-0.39258, -0.31128, 0.67374),
    (0.03308, 0.07616, 0.03422), (-0.31777, 0.1885, 0.40808), (-0.17464, 0.28096, 0.11686), (-0.50199, -0.49002, 0.2709),
    (0.38629, 0.15627, 0.56716), (0.06649, -0.05762, 0.0857), (-0.1065, -0.11726, 0.10818), (0.53236, -0.5286, 0.45444)], dtype=np.float32)


# ---- the shared pieces ---------------------------------------------------------------------------------------------------------
def mat4_mul(m, p, w):
    """column-major mat4 (m[c*4 + r]) times vec4(p, w): ((c0 x + c1 y) + c2 z) + c3 w, for (N, 3) p"""
    m = np.asarray(m, dtype=np.float32)
    w = F(w)
    return np.stack([((m[r] * p[:, 0] + m[4 + r] * p[:, 1]) + m[8 + r] * p[:, 2]) + m[12 + r] * w for r in range(4)], axis=-1)


def bilinear(img, x, y):
    """texture() of an RGBA32F image through LINEAR + MIRRORED_REPEAT at texel coordinates (x, y): rgb, (N, 3); beyond 1e9 texels 0"""
    H, W = img.shape[:2]
    ok = (np.abs(x) < F(1e9)) & (np.abs(y) < F(1e9))
    x, y = np.where(ok, x, F(0.0)), np.where(ok, y, F(0.0))
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[:, None], (y - fy)[:, None]
    mirror = lambda i, n: np.where(np.mod(i, 2 * n) < n, np.mod(i, 2 * n), 2 * n - 1 - np.mod(i, 2 * n))
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = mirror(ix, W), mirror(ix + 1, W), mirror(iy, H), mirror(iy + 1, H)
    t = lambda yy, xx: img[yy, xx, :3]
    a = t(y0, x0) * (F(1.0) - ax) + t(y0, x1) * ax
    b = t(y1, x0) * (F(1.0) - ax) + t(y1, x1) * ax
    return np.where(ok[:, None], a * (F(1.0) - ay) + b * ay, F(0.0))


def unorm16(x):
    x = np.where(x > 0, x, F(0.0))
    x = np.where(x > 1, F(1.0), x)
    return np.rint(x * F(65535.0)).astype(np.uint16)


def unorm_lut(c):
    return np.asarray(c).astype(np.float32) / F(255.0)


# ---- ssao_pass ------------------------------------------------------------------------------------------------------------------
def ssao(position, normal, view):
    """ssao.frag: (H, W) uint16. Texel (x, y) is the occlusion of G-buffer texel (x, H-1-y) (the unflipped in_uv), read exactly; the 32
    projected samples go through FLIP_UV_Y and read the position target bilinearly"""
    H, W = position.shape[:2]
    with np.errstate(all="ignore"):
        p = position[::-1, :, :3].reshape(-1, 3)
        nw = normal[::-1, :, :3].reshape(-1, 3)
        sky = (p[:, 0] == 1) & (p[:, 1] == 1) & (p[:, 2] == 1)
        frag = mat4_mul(view.view, p, 1.0)[:, :3]
        m = np.array(view.inverse_view[:], dtype=np.float32)
        nv = hr.normalize(np.stack([((m[4 * i] * nw[:, 0] + m[4 * i + 1] * nw[:, 1]) + m[4 * i + 2] * nw[:, 2]) + m[4 * i + 3] * F(0.0) for i in range(3)], axis=-1))
        rnd = np.array([1.0, 1.0, 0.0], np.float32)
        tangent = hr.normalize(rnd[None, :] - nv * hr.dot(rnd[None, :], nv)[:, None])
        bitangent = hr.cross(tangent, nv)
        o = np.zeros(len(p), np.float32)
        for k in range(32):
            kx, ky, kz = SSAO_KERNEL[k]
            sp = frag + ((tangent * kx + bitangent * ky) + nv * kz) * F(0.1)
            c = mat4_mul(view.projection, sp, 1.0)
            u = (c[:, 0] / c[:, 3]) * F(0.5) + F(0.5)
            v = F(1.0) - ((c[:, 1] / c[:, 3]) * F(0.5) + F(0.5))
            q = bilinear(position, u * F(W) - F(0.5), v * F(H) - F(0.5))
            depth = mat4_mul(view.view, q, 1.0)[:, 2]
            t = F(0.1) / np.abs(frag[:, 2] - depth)
            t = np.minimum(np.maximum(t, F(0.0)), F(1.0))
            rng = (t * t) * (F(3.0) - F(2.0) * t)
            o = o + np.where(depth >= sp[:, 2], F(1.0), F(0.0)) * rng
        occ = F(1.0) - (o / F(32.0)) * F(1.6)
        occ = np.where(sky, F(1.0), occ)
    return unorm16(occ).reshape(H, W)


# ---- deferred_pass --------------------------------------------------------------------------------------------------------------
def gamma_table():
    """pow(c / 255, 2.2) for every UNORM8 value: pow in double, rounded to float"""
    c = np.arange(256, dtype=np.float32) / F(255.0)
    return np.power(c.astype(np.float64), np.float64(F(2.2))).astype(np.float32)


def light_records(view, lights):
    """record 0: deferred.frag:74's sun; then the GpuLight records in order - (mode, pos, color, spot, att, dir) as the kernel's prep.
    Each record also carries `light`: the 24 floats of the Light that surfaceShading is handed (bindless.glsl's layout), untouched"""
    recs = []
    sun = np.array(view.sun_dir[:], dtype=np.float32)
    srcs = [dict(type=F(0.0), pos=np.zeros(3, np.float32), color=np.ones(3, np.float32), spot=F(0.0), att=np.ones(3, np.float32),
                 dir=sun * np.array([-1.0, 1.0, -1.0], np.float32))]
    for l in lights:
        srcs.append(dict(type=F(l.light_type), pos=np.array(l.position[:], np.float32), color=np.array(l.color[:3], np.float32), spot=F(l.spot),
                         att=np.array(l.attenuation[:], np.float32), dir=np.array(l.direction[:], np.float32)))
    raw = [np.array([1, 1, 1, 1, 0, 0, 0, 0, *srcs[0]["dir"], 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)]  # deferred.frag:74
    raw += [np.frombuffer(bytes(l), dtype=np.float32, count=24).copy() for l in lights]
    for s, light in zip(srcs, raw):
        t = s["type"]
        mode = 0 if t == 0 else 1 if t == 1 else 2 if t == 2 else 3
        d = np.zeros(3, np.float32)
        if t == 0:
            d = hr.normalize((s["dir"] * np.array([-1.0, 1.0, -1.0], np.float32))[None, :])[0]
        if t == 2:
            d = hr.normalize(s["dir"][None, :])[0]
        recs.append(dict(mode=mode, pos=s["pos"], color=s["color"], spot=s["spot"], att=s["att"], dir=d, light=light))
    return recs


def deferred(g, shadows, reflections, ssao_img, view, meshes, lights, surface_shading=None):
    """deferred.frag: (H, W, 4) float32 from the G-buffer targets `g` (dict of hybrid_reference.gbuffer's keys), the rt_shadows (H, W)
    and rt_reflections (H, W, 4) images, the SSAO image (H, W), the view and the GpuLight records (view.num_lights of them are used).
    surface_shading(position, base_color, normal, metallic, roughness, light, eye) -> (n, 3), with `light` the 24 floats of one Light,
    replaces the per-light term (pbr_lighting.glsl's surfaceShading at lightColorFactor 1); the default is this file's own reading of
    it. tests/test_ref_shaders.py runs the same glue over the reference's compiled text that way"""
    H, W = g["position"].shape[:2]
    n = H * W
    P, N, R = (g[k][..., :3].reshape(-1, 3) for k in ("position", "normal", "pbr"))
    R = g["pbr"].reshape(-1, 4)
    A = g["albedo"].reshape(-1, 4)
    material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    table = lambda key, default: np.where(valid, np.array([m[key] for m in meshes] or [default], np.float32)[idx], F(default))
    mf, rf, typ = table("metallic", 1.0), table("roughness", 1.0), table("type", 0.0)
    bc = np.where(valid[:, None], np.array([m["base_color"] for m in meshes] or [np.ones(3)], np.float32)[idx], F(1.0))
    with np.errstate(all="ignore"):
        roughness, metallic, occlusion = R[:, 1] * rf, R[:, 0] * mf, R[:, 2]
        diffuse = gamma_table()[A[:, :3]]
        base = diffuse * bc
        eye = np.array(view.eye_pos[:], np.float32)
        V = hr.normalize(eye[None, :] - P)
        om = F(1.0) - metallic
        F0 = np.full((n, 3), F(0.04), np.float32) * om[:, None] + base * metallic[:, None]
        NdotV = np.maximum(hr.dot(N, V), F(0.0))
        a = roughness * roughness
        a2 = a * a
        a2m1 = a2 - F(1.0)
        r1 = roughness + F(1.0)
        k = (r1 * r1) / F(8.0)
        omk = F(1.0) - k
        ggxV = NdotV / (NdotV * omk + k)
        nv4 = F(4.0) * NdotV
        Lo = np.zeros((n, 3), np.float32)
        for rec in light_records(view, list(lights)[: view.num_lights]):
            if surface_shading is not None:
                Lo = Lo + np.asarray(surface_shading(P, base, N, metallic, roughness, rec["light"], eye), np.float32)
                continue
            if rec["mode"] == 0:
                L, att = np.broadcast_to(rec["dir"], (n, 3)), np.ones(n, np.float32)
            elif rec["mode"] == 3:
                L, att = np.zeros((n, 3), np.float32), np.ones(n, np.float32)
            else:
                ptl = rec["pos"][None, :] - P
                d = np.sqrt(hr.dot(ptl, ptl))
                L = ptl * (F(1.0) / d)[:, None]
                at = rec["att"]
                den = (at[0] * F(1.0) + at[1] * d) + at[2] * (d * d)
                if rec["mode"] == 2:
                    att = np.power(np.maximum(hr.dot(L, rec["dir"][None, :]), F(0.0)), rec["spot"]) / den
                else:
                    att = F(1.0) / den
            Hv = hr.normalize(V + L)
            rad = rec["color"][None, :] * att[:, None]
            NdotH = np.maximum(hr.dot(N, Hv), F(0.0))
            dn = (NdotH * NdotH) * a2m1 + F(1.0)
            dn = (PI * dn) * dn
            NDF = a2 / dn
            NdotL = np.maximum(hr.dot(N, L), F(0.0))
            G = (NdotL / (NdotL * omk + k)) * ggxV
            x = np.minimum(np.maximum(F(1.0) - np.maximum(hr.dot(Hv, V), F(0.0)), F(0.0)), F(1.0))
            p5 = ((x * x) * (x * x)) * x
            Fr = F0 + (F(1.0) - F0) * p5[:, None]
            kD = (F(1.0) - Fr) * om[:, None]
            NG = NDF * G
            den2 = nv4 * NdotL + F(0.0001)
            spec = (NG[:, None] * Fr) / den2[:, None]
            c = (kD * base) / PI + spec
            Lo = Lo + (c * rad) * NdotL[:, None]
        color = (F(0.03) * diffuse) * occlusion[:, None] + Lo
        rt = view.raytracing_supported == 1
        if rt:
            refl = unorm_lut(reflections.reshape(-1, 4)[:, :3])
            metal = typ == 1.0
            color = np.where(metal[:, None], color * (F(1.0) - F(1.0)) + refl * F(1.0), color)
            color = color * np.maximum(unorm_lut(shadows.reshape(-1)), F(0.3))[:, None]
        if view.ssao_enabled == 1:
            color = color * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
    out = np.ones((n, 4), np.float32)
    out[:, :3] = color
    return out.reshape(H, W, 4)


# ---- atmosphere_pass ------------------------------------------------------------------------------------------------------------
def sky(position, view):
    """atmosphere.frag (cubemap off) on the G-buffer's miss pixels: {(y, x): rgb} along the un-jittered primary ray"""
    H, W = position.shape[:2]
    out = {}
    for y, x in zip(*np.nonzero(position[..., 3] == 0)):
        r = oa.primary_ray(view, W, H, int(x), int(y), 0.5, 0.5)
        out[(int(y), int(x))] = oa.sky(r[:3], r[3:], view.sun_dir[:])
    return out


# ---- present_pass ---------------------------------------------------------------------------------------------------------------
def linear_to_srgb(c):
    """view.glsl:53-61 with pow in double, rounded to float"""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(all="ignore"):
        p = np.power(c.astype(np.float64), np.float64(F(1.0) / F(2.4))).astype(np.float32)
        return np.where(c < F(0.0031308), c * F(12.92), F(1.055) * p - F(0.055))


def luma(rgb):
    return np.sqrt(hr.dot(rgb, np.array([0.299, 0.587, 0.114], np.float32)[None, :]))


def fxaa(img):
    """fxaa.glsl (enabled, no debug, threshold 0.45; SCREEN_WIDTH / HEIGHT 2000 x 1260) at every pixel centre: (H, W, 3) float32"""
    H, W = img.shape[:2]
    fW, fH = F(W), F(H)
    py, px = np.mgrid[0:H, 0:W]
    u = (px.reshape(-1).astype(np.float32) + F(0.5)) / fW
    v = (py.reshape(-1).astype(np.float32) + F(0.5)) / fH
    tex = lambda uu, vv: bilinear(img, uu * fW - F(0.5), vv * fH - F(0.5))
    off = lambda ox, oy: luma(bilinear(img, (u * fW + F(ox)) - F(0.5), (v * fH + F(oy)) - F(0.5)))
    center = tex(u, v)
    color = center.copy()
    with np.errstate(all="ignore"):
        lC = luma(center)
        lD, lU, lL, lR = off(0, -1), off(0, 1), off(-1, 0), off(1, 0)
        lMin = np.minimum(lC, np.minimum(np.minimum(lD, lU), np.minimum(lL, lR)))
        lMax = np.maximum(lC, np.maximum(np.maximum(lD, lU), np.maximum(lL, lR)))
        rng = lMax - lMin
        edge = ~(rng < np.maximum(F(0.0312), lMax * F(0.45)))
        lDL, lUR, lUL, lDR = off(-1, -1), off(1, 1), off(-1, 1), off(1, -1)
        lDU, lLR = lD + lU, lL + lR
        lLC, lDC, lRC, lUC = lDL + lUL, lDL + lDR, lDR + lUR, lUR + lUL
        eH = (np.abs(F(-2.0) * lL + lLC) + np.abs(F(-2.0) * lC + lDU) * F(2.0)) + np.abs(F(-2.0) * lR + lRC)
        eV = (np.abs(F(-2.0) * lU + lUC) + np.abs(F(-2.0) * lC + lLR) * F(2.0)) + np.abs(F(-2.0) * lD + lDC)
        horiz = eH >= eV
        l1, l2 = np.where(horiz, lD, lL), np.where(horiz, lU, lR)
        g1, g2 = l1 - lC, l2 - lC
        steep1 = np.abs(g1) >= np.abs(g2)
        gs = F(0.25) * np.maximum(np.abs(g1), np.abs(g2))
        isx, isy = F(1.0) / F(2000.0), F(1.0) / F(1260.0)
        step = np.where(horiz, isy, isx)
        step = np.where(steep1, -step, step)
        avg = np.where(steep1, F(0.5) * (l1 + lC), F(0.5) * (l2 + lC))
        cu = np.where(horiz, u, u + step * F(0.5))
        cv = np.where(horiz, v + step * F(0.5), v)
        ox, oy = np.where(horiz, isx, F(0.0)), np.where(horiz, F(0.0), isy)
        u1, v1, u2, v2 = cu - ox, cv - oy, cu + ox, cv + oy
        e1, e2 = luma(tex(u1, v1)) - avg, luma(tex(u2, v2)) - avg
        r1, r2 = np.abs(e1) >= gs, np.abs(e2) >= gs
        u1, v1 = np.where(r1, u1, u1 - ox), np.where(r1, v1, v1 - oy)
        u2, v2 = np.where(r2, u2, u2 + ox), np.where(r2, v2, v2 + oy)
        active = ~(r1 & r2)
        for q in (F(2.0), F(2.0), F(2.0), F(4.0), F(8.0)):  # QUALITY[2..6]
            e1 = np.where(active & ~r1, luma(tex(u1, v1)) - avg, e1)
            e2 = np.where(active & ~r2, luma(tex(u2, v2)) - avg, e2)
            r1 = np.where(active, np.abs(e1) >= gs, r1)
            r2 = np.where(active, np.abs(e2) >= gs, r2)
            m1, m2 = active & ~r1, active & ~r2
            u1, v1 = np.where(m1, u1 - ox * q, u1), np.where(m1, v1 - oy * q, v1)
            u2, v2 = np.where(m2, u2 + ox * q, u2), np.where(m2, v2 + oy * q, v2)
            active = active & ~(r1 & r2)
        d1 = np.where(horiz, u - u1, v - v1)
        d2 = np.where(horiz, u2 - u, v2 - v)
        dir1 = d1 < d2
        dmin, thick = np.minimum(d1, d2), d1 + d2
        pix_off = -dmin / thick + F(0.5)
        correct = (np.where(dir1, e1, e2) < F(0.0)) != (lC < avg)
        fo = np.where(correct, pix_off, F(0.0))
        lAvg = (F(1.0) / F(12.0)) * (((F(2.0) * (lDU + lLR)) + lLC) + lRC)
        s1 = np.minimum(np.maximum(np.abs(lAvg - lC) / rng, F(0.0)), F(1.0))
        s2 = ((F(-2.0) * s1 + F(3.0)) * s1) * s1
        fo = np.fmax(fo, (s2 * s2) * F(0.75))
        fu = np.where(horiz, u, u + fo * step)
        fv = np.where(horiz, v + fo * step, v)
        color = np.where(edge[:, None], tex(fu, fv), color)
    return color.reshape(H, W, 3)


def present(img, fxaa_enabled=True):
    """present.frag: (H, W, 4) uint8 B, G, R, A = 255 from the deferred output (H, W, 4) float32"""
    H, W = img.shape[:2]
    if fxaa_enabled:
        color = fxaa(img)
    else:
        u = (np.arange(W, dtype=np.float32) + F(0.5)) / F(W)
        v = (np.arange(H, dtype=np.float32) + F(0.5)) / F(H)
        uu, vv = np.meshgrid(u, v)
        color = bilinear(img, uu.reshape(-1) * F(W) - F(0.5), vv.reshape(-1) * F(H) - F(0.5)).reshape(H, W, 3)
    s = hr.unorm8(np.nan_to_num(linear_to_srgb(color), nan=0.0).astype(np.float32))
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = s[..., 2], s[..., 1], s[..., 0]
    return out

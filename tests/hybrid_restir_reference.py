"""CPU restatement of the hybrid frame's reservoir lights (uh_render_hybrid's UH_HYBRID_RESTIR_LIGHTS): which pixels cast a ray toward
the light of their spatial reservoir, the rays' verdicts, and the deferred pass with the sun plus that one light, in numpy float32 in the
order DESIGN.md section 2 "Reservoir lights" pins. Composed from tests/hybrid_reference.py (offset_ray, trace through the oracle's
trace_closest with the predicate "hit and t <= distance"), tests/hybrid_frame_reference.py (light_records and the pieces around the
light loop) and the oracle's reservoir passes. The deferred pass's arithmetic is restated here split where the kernel splits it - the
light-independent terms, then one light's term - and test_hybrid_restir_cpu.py holds the sum over all lights to
hybrid_frame_reference.deferred bit for bit. Each function takes its input images as arguments, so a test can feed it the device's own
G-buffer and reservoirs. Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import rust_renderer_amd as rr

F = np.float32
PI = fr.PI


# ---- the deferred pass's light loop, split as hybrid_shading.h splits it ---------------------------------------------------------
def surface_terms(g, view, meshes):
    """deferred.frag up to the light loop, per pixel (n = H * W rows): the G-buffer's own texels and surfaceShading's hoisted terms"""
    H, W = g["position"].shape[:2]
    n = H * W
    P, N = (g[k][..., :3].reshape(-1, 3) for k in ("position", "normal"))
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
        diffuse = fr.gamma_table()[A[:, :3]]
        base = diffuse * bc
        eye = np.array(view.eye_pos[:], np.float32)
        V = hr.normalize(eye[None, :] - P)
        om = F(1.0) - metallic
        F0 = np.full((n, 3), F(0.04), np.float32) * om[:, None] + base * metallic[:, None]
        NdotV = np.maximum(hr.dot(N, V), F(0.0))
        a = roughness * roughness
        a2 = a * a
        r1 = roughness + F(1.0)
        k = (r1 * r1) / F(8.0)
        omk = F(1.0) - k
    return dict(n=n, shape=(H, W), P=P, N=N, V=V, base=base, diffuse=diffuse, occlusion=occlusion, metallic=metallic, roughness=roughness,
                type=typ, om=om, F0=F0, a2=a2, a2m1=a2 - F(1.0),
                k=k, omk=omk, ggxV=NdotV / (NdotV * omk + k), nv4=F(4.0) * NdotV, geometry=g["position"].reshape(-1, 4)[:, 3] != 0)


def light_geometry(rec, P):
    """L and the distance of a point or spot light record at the points P: direct_lighting's ptl, d, L"""
    with np.errstate(all="ignore"):
        ptl = rec["pos"][None, :] - P
        d = np.sqrt(hr.dot(ptl, ptl))
        return ptl * (F(1.0) / d)[:, None], d


def light_term(s, rec, rows=None):
    """one iteration of the light loop on record `rec` (hybrid_frame_reference.light_records) for the pixels `rows` (all): c, rad, NdotL with
    Lo += (c * rad) * NdotL"""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    P, N, V, base, om, F0 = (pick(s[k]) for k in ("P", "N", "V", "base", "om", "F0"))
    a2, a2m1, k, omk, ggxV, nv4 = (pick(s[key]) for key in ("a2", "a2m1", "k", "omk", "ggxV", "nv4"))
    n = len(P)
    with np.errstate(all="ignore"):
        if rec["mode"] == 0:
            L, att = np.broadcast_to(rec["dir"], (n, 3)), np.ones(n, np.float32)
        elif rec["mode"] == 3:
            L, att = np.zeros((n, 3), np.float32), np.ones(n, np.float32)
        else:
            L, d = light_geometry(rec, P)
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
    return c, rad, NdotL


def finish(s, Lo, shadows, reflections, ssao_img, view):
    """deferred.frag after the light loop (no IBL, no shadow maps): ambient, the reflection mix, max(shadow, 0.3), SSAO; (H, W, 4)"""
    H, W = s["shape"]
    with np.errstate(all="ignore"):
        color = (F(0.03) * s["diffuse"]) * s["occlusion"][:, None] + Lo
        if view.raytracing_supported == 1:
            refl = fr.unorm_lut(reflections.reshape(-1, 4)[:, :3])
            metal = s["type"] == 1.0
            color = np.where(metal[:, None], color * (F(1.0) - F(1.0)) + refl * F(1.0), color)
            color = color * np.maximum(fr.unorm_lut(shadows.reshape(-1)), F(0.3))[:, None]
        if view.ssao_enabled == 1:
            color = color * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
    out = np.ones((s["n"], 4), np.float32)
    out[:, :3] = color
    return out.reshape(H, W, 4)


def sum_lights(s, recs):
    Lo = np.zeros((s["n"], 3), np.float32)
    with np.errstate(all="ignore"):
        for rec in recs:
            c, rad, NdotL = light_term(s, rec)
            Lo = Lo + (c * rad) * NdotL[:, None]
    return Lo


def deferred_all_lights(g, shadows, reflections, ssao_img, view, meshes, lights):
    """the plain deferred pass from the split pieces: equals hybrid_frame_reference.deferred bit for bit"""
    s = surface_terms(g, view, meshes)
    return finish(s, sum_lights(s, fr.light_records(view, list(lights)[: view.num_lights])), shadows, reflections, ssao_img, view)


# ---- the restir_lights pass ------------------------------------------------------------------------------------------------------
def cast_mask(g, res, view, lights):
    """(H, W) bool: the pixels that cast a ray - geometry, 0 <= Y < view.num_lights, a point or spot light, W_X finite and > 0, and the
    light's NdotL (direct_lighting's own expressions; NaN counts as culled) not 0"""
    H, W = g["position"].shape[:2]
    P, N = (g[k][..., :3].reshape(-1, 3) for k in ("position", "normal"))
    Y, WX = res["Y"].reshape(-1), res["W_X"].reshape(-1)
    nl = min(int(view.num_lights), len(lights))
    recs = fr.light_records(view, list(lights)[:nl])[1:]
    ok = (g["position"].reshape(-1, 4)[:, 3] != 0) & (Y >= 0) & (Y < nl) & np.isfinite(WX) & (WX > 0)
    cast = np.zeros(H * W, bool)
    for j, rec in enumerate(recs):
        rows = np.nonzero(ok & (Y == j))[0]
        if rec["mode"] not in (1, 2) or not len(rows):
            continue
        L, _ = light_geometry(rec, P[rows])
        with np.errstate(all="ignore"):
            ndl = np.fmax(hr.dot(N[rows], L), F(0.0))  # fmaxf: NaN gives 0
        cast[rows] = ndl != 0
    return cast.reshape(H, W)


def shadow_rays(g, rows, light_pos):
    """make_shadow_ray<true> (reference.rgen:113-114) from offset_ray(P, N) of pixels `rows` toward light_pos (len(rows), 3): origins,
    directions, distances"""
    P, N = (g[k][..., :3].reshape(-1, 3)[rows] for k in ("position", "normal"))
    o = hr.offset_ray(P, N)
    to = light_pos - o
    with np.errstate(all="ignore"):
        return o, hr.normalize(to), np.sqrt(hr.dot(to, to))


def occluded(oracle, o, d, dist):
    """some triangle has 0.001 < t < 10000 and t <= dist: the closest hit decides"""
    t, _, _, mesh, _ = hr.trace(oracle, o, d)
    return (mesh != hr.MISS) & (t <= dist)


def visibility(oracle, g, res, view, lights):
    """the light-visibility image (H, W) uint8, the rays cast and the occluded ones"""
    H, W = g["position"].shape[:2]
    cast = cast_mask(g, res, view, lights).reshape(-1)
    rows = np.nonzero(cast)[0]
    vis = np.zeros(H * W, np.uint8)
    if len(rows):
        pos = np.array([l.position[:] for l in lights], np.float32).reshape(-1, 3)[res["Y"].reshape(-1)[rows]]
        occ = occluded(oracle, *shadow_rays(g, rows, pos))
        vis[rows] = np.where(occ, 0, 255)
    else:
        occ = np.zeros(0, bool)
    return vis.reshape(H, W), len(rows), int(occ.sum())


def reservoir_term(s, view, lights, res, vis):
    """((c * rad) * NdotL) * W_X of light record Y + 1 where the visibility texel is 255, else 0; (n, 3) and the mask"""
    Y, WX = res["Y"].reshape(-1), res["W_X"].reshape(-1)
    lit = vis.reshape(-1) == 255
    recs = fr.light_records(view, list(lights)[: view.num_lights])
    term = np.zeros((s["n"], 3), np.float32)
    with np.errstate(all="ignore"):
        for j in np.unique(Y[lit]):
            rows = np.nonzero(lit & (Y == j))[0]
            c, rad, NdotL = light_term(s, recs[int(j) + 1], rows)
            term[rows] = ((c * rad) * NdotL[:, None]) * WX[rows, None]
    return term, lit


def deferred(g, shadows, reflections, ssao_img, view, meshes, lights, res, vis):
    """the deferred pass with the bit: Lo = Lo_sun, then Lo = Lo + term where the visibility texel is 255; (H, W, 4) float32"""
    s = surface_terms(g, view, meshes)
    Lo = sum_lights(s, fr.light_records(view, [])[:1])
    term, lit = reservoir_term(s, view, lights, res, vis)
    with np.errstate(all="ignore"):
        Lo = np.where(lit[:, None], Lo + term, Lo)
    return finish(s, Lo, shadows, reflections, ssao_img, view)


# ---- what the estimator estimates ------------------------------------------------------------------------------------------------
def all_lights_visibility(oracle, g, view, lights):
    """per light j < view.num_lights: (rows, visible) over the geometry pixels whose NdotL toward light j is not 0 - the pairs a ray
    could be cast for - with the oracle's visibility of each"""
    s_geo = g["position"].reshape(-1, 4)[:, 3] != 0
    P, N = (g[k][..., :3].reshape(-1, 3) for k in ("position", "normal"))
    out = []
    for rec, l in zip(fr.light_records(view, list(lights)[: view.num_lights])[1:], lights):
        if rec["mode"] not in (1, 2):
            out.append((np.zeros(0, np.int64), np.zeros(0, bool)))
            continue
        L, _ = light_geometry(rec, P)
        with np.errstate(all="ignore"):
            rows = np.nonzero(s_geo & (np.fmax(hr.dot(N, L), F(0.0)) != 0))[0]
        pos = np.broadcast_to(np.array(l.position[:], np.float32), (len(rows), 3))
        out.append((rows, ~occluded(oracle, *shadow_rays(g, rows, pos))))
    return out


def brute_force_sum(s, view, lights, pairs, shadowed=True):
    """sum over pixels and lights of term_i * V_i (float64 accumulation of the float32 terms), per channel; shadowed=False drops V"""
    total = np.zeros(3, np.float64)
    recs = fr.light_records(view, list(lights)[: view.num_lights])[1:]
    for rec, (rows, visible) in zip(recs, pairs):
        if not len(rows):
            continue
        c, rad, NdotL = light_term(s, rec, rows)
        t = ((c * rad) * NdotL[:, None]).astype(np.float64)
        total += t[visible].sum(axis=0) if shadowed else t.sum(axis=0)
    return total


# ---- lights for the tests --------------------------------------------------------------------------------------------------------
def occluded_lights(n=16):
    """n point and spot lights behind the synthetic scene's three occluders as the camera sees them (the ellipsoid about (-1.5, 0.8, 0),
    the quad about (2.2, 1, -1), the metal sphere about (0.6, 0.7, 1.4)), a little above them: the floor the camera sees in front of an
    occluder lies in its shadow. make_light's attenuation (0, 0, 0.1) falls off as the reservoirs' target function does, 1 / d^2, which
    keeps the estimator's variance down."""
    anchors = [(-1.5, 0.0), (2.2, -1.0), (0.6, 1.4)]
    lights = []
    for k in range(n):
        ax, az = anchors[k % 3]
        a = np.pi * (0.15 + 0.7 * ((k // 3) + 0.5) / 6.0)
        radius = 1.8 + 0.25 * (k % 4)
        l = rr.make_light((ax + radius * np.cos(a), 1.3 + 0.15 * (k % 3), az - radius * np.sin(a)),
                          color=(0.3 + 0.7 * ((k * 5) % 7) / 6.0, 0.9 - 0.6 * ((k * 3) % 5) / 4.0, 0.4 + 0.5 * (k % 3) / 2.0))
        l.light_type = float(1 + k % 2)
        l.direction[:] = (-np.cos(a), -0.2, np.sin(a))  # the spot lights look at their occluder
        l.spot = 1.0 + (k % 2)
        lights.append(l)
    return lights

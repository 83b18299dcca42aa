"""A float64 reading of the hybrid frame's SSAO, deferred and present passes, written from the shaders and not from the float32
restatements: deferred.frag:43-118, pbr_lighting.glsl:20-108 (surfaceShading, imageBasedLighting), brdf.glsl:1-36 and 82-90,
shadow_mapping.glsl:8-54 (calculateShadow), the reservoir light's term of DESIGN.md section 2 "Reservoir lights", ssao.frag:
66-118, present.frag:23-39 with view.glsl:53-66 (linearToSrgb), and the samplers they read through (texture.rs: LINEAR +
MIRRORED_REPEAT; the IBL cubes with the Vulkan face table and seamless edges of DESIGN.md section 2). Only the inputs are shared with
tests/hybrid_frame_reference.py and tests/ibl_reference.py (the recorded meshes and the read-back maps); no arithmetic is.

GLSL float literals are single precision, so each constant enters as its float32 value (F(0.04), F(2.2), ...); every operation on them
is float64. What the passes read (G-buffer words, UNORM texels, the fp16 LUT, the cubes' float32 texels) is taken exactly.
Not a conftest: test modules import it."""
import numpy as np

D = np.float64
F = np.float32


def c(x):
    """a GLSL float literal: its float32 value, in float64"""
    return D(F(x))


PI = c(3.14159265359)  # brdf.glsl:1


def dot(a, b):
    return np.sum(a * b, axis=-1)


def normalize(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return a / np.sqrt(dot(a, a))[..., None]


def mirror(i, n):
    """MIRRORED_REPEAT texel index"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def bilinear(img, x, y):
    """LINEAR + MIRRORED_REPEAT at texel coordinates x = u W - 0.5, y = v H - 0.5 of img (H, W, C): (N, C) float64; a coordinate
    beyond 1e9 texels (as the device's sampler) or not finite reads 0"""
    H, W = img.shape[:2]
    x, y = np.asarray(x, D), np.asarray(y, D)
    ok = (np.abs(x) < 1e9) & (np.abs(y) < 1e9)
    x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[:, None], (y - fy)[:, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = mirror(ix, W), mirror(ix + 1, W), mirror(iy, H), mirror(iy + 1, H)
    t = lambda yy, xx: img[yy, xx].astype(D)
    v = (t(y0, x0) * (1 - ax) + t(y0, x1) * ax) * (1 - ay) + (t(y1, x0) * (1 - ax) + t(y1, x1) * ax) * ay
    return np.where(ok[:, None], v, 0.0)


# ---- cube maps (Vulkan 16.5.4 face selection; seamless edges and the corner rule of DESIGN.md section 2) ------------------------------
# face: (major axis, its sign, sc axis, sc sign, tc axis, tc sign), from the Vulkan table: +X sc -z tc -y, -X +z -y, +Y +x +z,
# -Y +x -z, +Z +x -y, -Z -x -y
VK_FACES = [(0, 1, 2, -1, 1, -1), (0, -1, 2, 1, 1, -1), (1, 1, 0, 1, 2, 1), (1, -1, 0, 1, 2, -1), (2, 1, 0, 1, 1, -1), (2, -1, 0, -1, 1, -1)]


def cube_face(d):
    """face and (s, t) in [0, 1] of directions d (N, 3): major axis the largest |component| (ties: x, then y; +0 and -0 positive)"""
    a = np.abs(d)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    neg = np.take_along_axis(d, axis[:, None], 1)[:, 0] < 0
    face = 2 * axis + neg
    s, t = np.empty(len(d)), np.empty(len(d))
    with np.errstate(divide="ignore", invalid="ignore"):
        for f, (ma, _, sa, ss, ta, ts) in enumerate(VK_FACES):
            sel = face == f
            m = np.abs(d[sel, ma])
            s[sel] = 0.5 * (ss * d[sel, sa] / m + 1.0)
            t[sel] = 0.5 * (ts * d[sel, ta] / m + 1.0)
    return face, s, t


def neighbour_texel(f, i, j, S):
    """the texel a seamless filter reads at (i, j) of face f when one of i, j is -1 or S: the centre of that would-be texel on the
    cube of half-size S, projected onto the face it points into, read at the nearest texel centre there. Returns (face, i, j)"""
    ma, ms, sa, ss, ta, ts = VK_FACES[f]
    P = np.zeros(3)
    P[ma], P[sa], P[ta] = ms * S, ss * (2 * i + 1 - S), ts * (2 * j + 1 - S)
    g = int(np.argmax(np.abs(P)))
    gf = 2 * g + (P[g] < 0)
    Q = P * (S / abs(P[g]))
    _, _, ga, gs, gt, gts = VK_FACES[gf]
    return gf, int(np.rint((gs * Q[ga] + S - 1) / 2)), int(np.rint((gts * Q[gt] + S - 1) / 2))


def cube_texel(level, f, i, j):
    """one texel (rgb, float64) at (i, j) in [-1, S]^2 of face f of level (6, S, S, 4); outside in both: the mean of the three texels
    that meet at that corner"""
    S = level.shape[1]
    oi, oj = not 0 <= i < S, not 0 <= j < S
    if not (oi or oj):
        return level[f, j, i, :3].astype(D)
    if oi and oj:
        ci, cj = min(max(i, 0), S - 1), min(max(j, 0), S - 1)
        a, b = neighbour_texel(f, i, cj, S), neighbour_texel(f, ci, j, S)
        return (level[f, cj, ci, :3].astype(D) + level[a[0], a[2], a[1], :3] + level[b[0], b[2], b[1], :3]) / 3.0
    g, gi, gj = neighbour_texel(f, i, j, S)
    return level[g, gj, gi, :3].astype(D)


def cube_bilinear(level, d):
    """texture(cube, d) at one level: (N, 3) float64; a direction with no face reads 0"""
    S = level.shape[1]
    out = np.zeros((len(d), 3))
    good = np.isfinite(d).all(axis=1) & (np.abs(d).max(axis=1) > 0)
    face, s, t = cube_face(np.where(good[:, None], d, 1.0))
    x, y = s * S - 0.5, t * S - 0.5
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
    inner = good & (i0 >= 0) & (j0 >= 0) & (i0 + 1 < S) & (j0 + 1 < S)
    lv = level[..., :3].astype(D)
    k = np.nonzero(inner)[0]
    f_, a_, b_ = face[k], i0[k], j0[k]
    t00, t10, t01, t11 = lv[f_, b_, a_], lv[f_, b_, a_ + 1], lv[f_, b_ + 1, a_], lv[f_, b_ + 1, a_ + 1]
    wx, wy = ax[k, None], ay[k, None]
    out[k] = (t00 * (1 - wx) + t10 * wx) * (1 - wy) + (t01 * (1 - wx) + t11 * wx) * wy
    for q in np.nonzero(good & ~inner)[0]:
        f, a, b = int(face[q]), int(i0[q]), int(j0[q])
        wx, wy = ax[q], ay[q]
        T = [cube_texel(level, f, a + di, b + dj) for dj in (0, 1) for di in (0, 1)]
        out[q] = (T[0] * (1 - wx) + T[1] * wx) * (1 - wy) + (T[2] * (1 - wx) + T[3] * wx) * wy
    return out


def cube_lod(levels, d, lod):
    """textureLod: lod clamped to [0, last], trilinear between floor(lod) and the next level"""
    lod = np.clip(np.broadcast_to(np.asarray(lod, D), (len(d),)), 0.0, len(levels) - 1)
    fl = np.floor(lod)
    m0 = fl.astype(np.int64)
    m1 = np.minimum(m0 + 1, len(levels) - 1)
    w = (lod - fl)[:, None]
    out = np.zeros((len(d), 3))
    for m in range(len(levels)):
        sel = m0 == m
        if sel.any():
            out[sel] += cube_bilinear(levels[m], d[sel]) * (1 - w[sel])
        sel = (m1 == m) & (w[:, 0] > 0)
        if sel.any():
            out[sel] += cube_bilinear(levels[m], d[sel]) * w[sel]
    return out


def lut_lookup(lut, u, v):
    """texture(in_brdf_lut, (u, v)): the fp16 (512, 512, 2) LUT, LINEAR + MIRRORED_REPEAT"""
    n = lut.shape[0]
    return bilinear(lut.astype(D), np.asarray(u, D) * n - 0.5, np.asarray(v, D) * n - 0.5)


# ---- deferred.frag -------------------------------------------------------------------------------------------------------------
# The float32 pass rounds ~40 operations per light and per ambient term, each within 2^-24 relative of its operands, and the terms of
# Lo are all >= 0: away from cancellation the error of a pixel is a small multiple of 2^-24 times its magnitude scale, ambient plus
# the sum of the per-light contributions. The cancellations are in the dot products the shader clamps and feeds on: NdotL, NdotV,
# NdotH, dot(H, V) and the spot cosine are dots of unit vectors, each with an absolute error of a few 2^-24. Their effect is measured
# here, not modelled: `sens` is the sum, over lights and those five inputs, of how far the float64 contribution moves when the input
# moves by DOT_ULPS 2^-24. It is large in the GGX peak (tiny a2, NdotH -> 1: dn = NdotH^2 (a2 - 1) + 1 cancels), for steep spot
# exponents, and where NdotL or NdotV is within rounding of 0. kappa = sens / (2^-24 scale) is the pixel's condition estimate.
# * well-conditioned pixels (kappa <= 64): |device - f64| <= 256 ulp of the scale (128 for the roundings, 2 x 64 for the inputs);
# * the others: <= 128 ulp of the scale + 2 sens (sens is first order in an input error taken at its largest).
ULP = 2.0 ** -24
DOT_ULPS = 4
KAPPA_WELL = 64.0
WELL_ULPS, PEAK_ULPS, PEAK_SENS = 256, 128, 2.0


def _material(pbr, meshes):
    material = np.floor(pbr[:, 3]).astype(np.int64)  # uint(texture(...).a): truncation; the values are >= 0
    valid = (material >= 0) & (material < len(meshes))
    idx = np.where(valid, material, 0)
    col = lambda key, default: np.where(valid, np.array([D(m[key]) for m in meshes] or [default], D)[idx], default)
    bc = np.array([np.asarray(m["base_color"], D)[:3] for m in meshes] or [np.ones(3)], D)[idx]
    return col("metallic", 1.0), col("roughness", 1.0), col("type", 0.0), np.where(valid[:, None], bc, 1.0)


def image_based_lighting(maps, P, base, N, metallic, roughness, occlusion, eye):
    """pbr_lighting.glsl:81-108 on the maps dict(irr=(6,S,S,4), spec=[levels], lut=(512,512,2) fp16): (N, 3) float64"""
    with np.errstate(all="ignore"):
        V = normalize(eye[None, :] - P)
        R = -(V - 2.0 * dot(N, V)[:, None] * N)                           # -reflect(V, N)
        F0 = c(0.04) * (1 - metallic)[:, None] + base * metallic[:, None]  # mix(0.04, base, metallic)
        NdotV = np.maximum(dot(N, V), 0.0)
        x5 = np.clip(1.0 - NdotV, 0.0, 1.0) ** 5
        Fr = F0 + (np.maximum((1.0 - roughness)[:, None], F0) - F0) * x5[:, None]  # fresnelSchlickRoughness
        kD = (1.0 - Fr) * (1 - metallic)[:, None]
        irradiance = cube_bilinear(maps["irr"], N)
        pre = cube_lod(maps["spec"], R, roughness * c(7.0))
        brdf = lut_lookup(maps["lut"], NdotV, 1.0 - roughness)
        spec = pre * (Fr * brdf[:, 0:1] + brdf[:, 1:2])
        return (kD * irradiance * base + spec) * occlusion[:, None]


def deferred(g, shadows, reflections, ssao_img, view, meshes, lights, maps=None, shadow=None, res=None, vis=None):
    """deferred.frag in float64 on the pass's own inputs (G-buffer dict of position / normal / albedo / pbr, the rt_shadows, rt_reflections
    and SSAO images, the view, the recorded meshes, the GpuLight records; the IBL maps when view.ibl_enabled). shadow = (params, maps):
    calculateShadow's factor in place of the rt_shadows factor (shadows_enabled = 1). res, vis (the spatial reservoirs and the
    light-visibility image, UH_HYBRID_RESTIR_LIGHTS): the loop runs over the sun alone, and a pixel whose visibility texel is 255 adds the
    term of light res.Y times res.W_X. Returns (color, scale, sens, kappa): color (H, W, 3), the per-channel magnitude scales (H, W, 3)
    and the condition estimate (H, W). With `shadow` the factor is an interval (shadow_interval), and color, scale and sens have a
    leading axis of 2: the values at the factor's lower and upper end"""
    H, W = g["position"].shape[:2]
    n = H * W
    P = g["position"][..., :3].reshape(-1, 3).astype(D)
    N = g["normal"][..., :3].reshape(-1, 3).astype(D)
    pbr = g["pbr"].reshape(-1, 4).astype(D)
    mf, rf, typ, bc = _material(pbr, meshes)
    roughness, metallic, occlusion = pbr[:, 1] * rf, pbr[:, 0] * mf, pbr[:, 2]
    diffuse = (g["albedo"].reshape(-1, 4)[:, :3].astype(D) / 255.0) ** c(2.2)  # frag:61
    base = diffuse * bc
    eye = np.array(view.eye_pos[:], D)
    srcs = [(0.0, np.zeros(3), np.ones(3), 0.0, np.ones(3), np.array(view.sun_dir[:], D) * (-1, 1, -1))]  # frag:74
    table = [(D(l.light_type), np.array(l.position[:], D), np.array(l.color[:3], D), D(l.spot), np.array(l.attenuation[:], D), np.array(l.direction[:], D))
             for l in list(lights)[: view.num_lights]]
    if res is None:
        srcs += table
    with np.errstate(all="ignore"):
        V = normalize(eye[None, :] - P)                                   # lighting:26
        F0 = c(0.04) * (1 - metallic)[:, None] + base * metallic[:, None]
        NdotV = np.maximum(dot(N, V), 0.0)
        a2 = roughness ** 4                                               # brdf:5-6
        k = (roughness + 1.0) ** 2 / 8.0                                  # brdf:19-20
        ggx = lambda x: x / (x * (1.0 - k) + k)
        Lo, scale, sens = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))

        def one_light(typ_l, pos, color, spot, att, ldir):
            """(lo, sens) of one light at every pixel: its contribution to Lo and how far that moves with its five dot products"""
            cos_s, spot_l, den = np.ones(n), 0.0, np.ones(n)
            if typ_l == 0.0:                                              # lighting:36-40
                L = np.broadcast_to(normalize((ldir * (-1, 1, -1))[None, :]), (n, 3))
            elif typ_l in (1.0, 2.0):                                     # lighting:41-53
                ptl = pos[None, :] - P
                d = np.sqrt(dot(ptl, ptl))
                L = normalize(ptl)
                den = att[0] + att[1] * d + att[2] * d * d
                if typ_l == 2.0:
                    cos_s, spot_l = dot(L, normalize(ldir[None, :])), spot
            else:
                L = np.zeros((n, 3))
            Hv = normalize(V + L)                                         # lighting:58
            x = dict(NL=dot(N, L), NV=dot(N, V), NH=dot(N, Hv), HV=dot(Hv, V), cs=cos_s)

            def contribution(NL, NV, NH, HV, cs):
                NdotL, NdotV, NdotH = np.maximum(NL, 0.0), np.maximum(NV, 0.0), np.maximum(NH, 0.0)
                attenuation = (np.maximum(cs, 0.0) ** spot_l if typ_l == 2.0 else 1.0) / den
                radiance = color[None, :] * attenuation[:, None]
                dn = NdotH * NdotH * (a2 - 1.0) + 1.0                     # brdf:3-15
                NDF = a2 / (PI * dn * dn)
                G = ggx(NdotL) * ggx(NdotV)                               # brdf:28-36
                Fr = F0 + (1.0 - F0) * (np.clip(1.0 - np.maximum(HV, 0.0), 0.0, 1.0) ** 5)[:, None]  # brdf:82-85
                kD = (1.0 - Fr) * (1.0 - metallic)[:, None]               # lighting:66-68
                spec = (NDF * G)[:, None] * Fr / (4.0 * NdotV * NdotL + c(0.0001))[:, None]
                return (kD * base / PI + spec) * radiance * NdotL[:, None]  # lighting:76

            lo = contribution(**x)
            moves = np.zeros((n, 3))
            for key in x:
                for sign in (-1.0, 1.0):
                    moved = dict(x, **{key: x[key] + sign * DOT_ULPS * ULP})
                    moves = moves + np.abs(np.nan_to_num(contribution(**moved) - lo, nan=0.0)) * 0.5
            return lo, moves

        for src in srcs:
            lo, moves = one_light(*src)
            Lo, scale, sens = Lo + lo, scale + np.abs(lo), sens + moves
        if res is not None:  # DESIGN.md section 2 "Reservoir lights": Lo += term(light Y) * W_X where the ray arrived
            Y, WX = res["Y"].reshape(-1), res["W_X"].reshape(-1).astype(D)
            arrived = vis.reshape(-1) == 255
            for j in np.unique(Y[arrived]):
                lo, moves = one_light(*table[int(j)])
                rows = (arrived & (Y == j))[:, None]
                lo, moves = np.where(rows, lo * WX[:, None], 0.0), np.where(rows, moves * WX[:, None], 0.0)
                Lo, scale, sens = Lo + lo, scale + np.abs(lo), sens + moves
        if view.ibl_enabled == 1:
            ambient = image_based_lighting(maps, P, base, N, metallic, roughness, occlusion, eye)
        else:
            ambient = c(0.03) * diffuse * occlusion[:, None]              # frag:83
        color = ambient + Lo                                              # frag:90
        scale = scale + np.abs(ambient)
        if view.raytracing_supported == 1:                                # frag:92-95, 108-111
            metal = (typ == 1.0)[:, None]
            refl = reflections.reshape(-1, 4)[:, :3].astype(D) / 255.0
            color = np.where(metal, color * 0.0 + refl, color)
            scale, sens = np.where(metal, refl, scale), np.where(metal, 0.0, sens)
        if shadow is not None:                                            # frag:98-106: calculateShadow, not rt_shadows
            s = np.stack(shadow_interval(P, view, *shadow)[:2])[:, :, None]  # (2, n, 1)
            color, scale, sens = color[None] * s, scale[None] * s, sens[None] * s
        elif view.raytracing_supported == 1:
            s = np.maximum(shadows.reshape(-1).astype(D) / 255.0, c(0.3))[:, None]
            color, scale, sens = color * s, scale * s, sens * s
        if view.ssao_enabled == 1:                                        # frag:55, 113-115: in_ssao at the unflipped in_uv
            s = (ssao_img[::-1].reshape(-1).astype(D) / 65535.0)[:, None]
            color, scale, sens = color * s, scale * s, sens * s
        kappa = np.nan_to_num(np.max((sens / (ULP * scale)).reshape(-1, n, 3)[-1], axis=1), nan=0.0, posinf=np.inf)  # (a factor cancels)
    shape = color.shape[:-2] + (H, W, 3)
    return color.reshape(shape), scale.reshape(shape), sens.reshape(shape), kappa.reshape(H, W)


def deferred_bound(scale, sens, kappa):
    """the stated bound on |device - f64| per channel (see above): which of the two applies is chosen by kappa"""
    peak = (kappa > KAPPA_WELL)[..., None]
    return np.where(peak, PEAK_ULPS * ULP * scale + PEAK_SENS * sens, WELL_ULPS * ULP * scale)


def worst_ratio(err, bound):
    """max of err / bound, 0 / 0 counting as 0 and x / 0 as infinite"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def interval_error(got, color, scale, sens, kappa):
    """(err, bound) of device values `got` (H, W, 3) against the reading: |got - color| and deferred_bound, or with a factor interval
    (a leading axis of 2 on color, scale and sens) the distance below the lower end against the bound there, or above the upper end
    against the bound there; inside the interval the error is 0"""
    if color.ndim == 3:
        return np.abs(got - color), deferred_bound(scale, sens, kappa)
    b = deferred_bound(scale, sens, kappa)
    below, above = color[0] - got, got - color[1]
    return np.where(below > 0, below, np.where(above > 0, above, 0.0)), np.where(below > 0, b[0], b[1])


# ---- shadow_mapping.glsl: calculateShadow ----------------------------------------------------------------------------------------
# The factor is a step function of three comparisons, so it is read as an interval [lo, hi] (as ssao() reads its depth comparisons): a
# comparison whose two sides lie within the float32 pass's own rounding of each other may go either way. The roundings are counted,
# not fitted; u = 2^-24 is the relative error of one float32 operation.
# * A row of a 4 x 4 matrix times (P, 1), ((m0 x + m1 y) + m2 z) + m3: three products and three sums (m3 * 1 is exact), each within
#   u of an intermediate no larger than A = |m0 x| + |m1 y| + |m2 z| + |m3|: SHADOW_ROW_ROUNDINGS u A absolute. This is the whole
#   error of viewPosition.z against the cascade splits (which are read exactly).
# * projCoordinate = lightSpacePosition / w: one more rounding of the quotient (w is 1, but the operation is counted).
# * The depth side: z - bias, one rounding. So testDepth errs by at most 6 u A_z + u |z| + u |z - bias|; the same without the last
#   term for z against the (-1, 1] ends.
# * The uv scale: xy * 0.5 + 0.5 (the product is exact, the sum rounds), and for v the flip 1 - v; then (uv + offset) * S - 0.5 with
#   1 / S rounded: a sum, a product and a sum. In texels, with |uv| <= 2 wherever a texel is read:
#   S (0.5 (6 u A_xy + u |p|) + u |uv| + u |uv| (flip) + u / S + u |uv + offset|) + u |t + 0.5| + u |t|
#   <= S (3 u A_xy + SHADOW_UV_ROUNDINGS u max(|uv|, |p|, 1)) + 2 u (|t| + 1).
# * The blend of four depths in [0, 1]: 1 - a, two products and a sum per axis, twice: SHADOW_BLEND_ROUNDINGS u of a value <= 1.
#   The blend is continuous in the texel coordinate, so the coordinate's error moves it by what the blend itself changes over a box of
#   that half-width: evaluated at the box's corners.
SHADOW_ROW_ROUNDINGS = 6
SHADOW_UV_ROUNDINGS = 5
SHADOW_BLEND_ROUNDINGS = 8


def _row(m, r, P):
    """row r of the column-major float32 matrix m (16,) times (P, 1): the value and A, the sum of the terms' magnitudes"""
    terms = np.stack([D(m[r]) * P[:, 0], D(m[4 + r]) * P[:, 1], D(m[8 + r]) * P[:, 2], np.full(len(P), D(m[12 + r]))])
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def _depth_bilinear(layer, x, y):
    return bilinear(layer[..., None], x, y)[:, 0]


def _cascade_interval(P, vp, layer):
    """the factor's interval for positions P (n, 3) in one cascade: vp (16,) float32, layer (S, S) float32"""
    S = layer.shape[0]
    (lx, ax), (ly, ay), (lz, az), (lw, _) = (_row(vp, r, P) for r in range(4))
    px, py, pz = lx / lw, ly / lw, lz / lw                                # shadow_mapping.glsl:19-20
    u, v = px * 0.5 + 0.5, 1.0 - (py * 0.5 + 0.5)                         # :21-22
    e_z = SHADOW_ROW_ROUNDINGS * ULP * az + ULP * np.abs(pz)
    e_test = e_z + ULP * np.abs(pz - c(0.0005))
    texel = 1.0 / S                                                       # :25
    lo, hi = np.zeros(len(P)), np.zeros(len(P))
    surely_in = (pz + e_z <= 1.0) & (pz - e_z > -1.0)                     # :33
    maybe_in = (pz - e_z <= 1.0) & (pz + e_z > -1.0)
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            uu, vv = u + ox * texel, v + oy * texel                       # :35-36
            tx, ty = uu * S - 0.5, vv * S - 0.5
            dx = S * (3 * ULP * ax + SHADOW_UV_ROUNDINGS * ULP * np.maximum(np.maximum(np.abs(uu), np.abs(px)), 1.0)) + 2 * ULP * (np.abs(tx) + 1.0)
            dy = S * (3 * ULP * ay + SHADOW_UV_ROUNDINGS * ULP * np.maximum(np.maximum(np.abs(vv), np.abs(py)), 1.0)) + 2 * ULP * (np.abs(ty) + 1.0)
            depths = [_depth_bilinear(layer, tx + sx * dx, ty + sy * dy) for sx in (-1, 1) for sy in (-1, 1)] + [_depth_bilinear(layer, tx, ty)]
            dmin = np.min(depths, axis=0) - SHADOW_BLEND_ROUNDINGS * ULP
            dmax = np.max(depths, axis=0) + SHADOW_BLEND_ROUNDINGS * ULP
            test = pz - c(0.0005)                                         # :37-39
            shadowed, lit = test - e_test > dmax, test + e_test < dmin    # :40: testDepth > closestDepth
            t_lo = np.where(lit, 1.0, c(0.3))
            t_hi = np.where(shadowed, c(0.3), 1.0)
            lo = lo + np.where(maybe_in, t_lo, 1.0)                       # :44: outside the frustum's depth no shadowing
            hi = hi + np.where(surely_in, t_hi, 1.0)
    return lo / 9.0, hi / 9.0                                             # :51


def shadow_interval(P, view, params, maps):
    """calculateShadow in float64 for world positions P (n, 3): (lo, hi, cascade_lo, cascade_hi). [lo, hi] holds the float32 pass's
    factor; a view depth within its rounding of a split takes the union over both cascades (cascade_lo .. cascade_hi)"""
    P = np.asarray(P, D)
    splits = np.array(params.cascade_splits[:], D)
    vps = [np.array(list(params.view_projection_matrices[k]), F) for k in range(4)]
    with np.errstate(all="ignore"):
        vz, a = _row(np.array(view.view[:], F), 2, P)                     # :11
        e = SHADOW_ROW_ROUNDINGS * ULP * a
        c_lo = sum((vz + e < -splits[i]).astype(np.int64) for i in range(3))  # :13-17: the splits ascend, so the last i that holds is the count
        c_hi = sum((vz - e < -splits[i]).astype(np.int64) for i in range(3))
        lo, hi = np.full(len(P), np.inf), np.full(len(P), -np.inf)
        for k in range(4):
            rows = np.nonzero((c_lo <= k) & (k <= c_hi))[0]
            if len(rows):
                l, h = _cascade_interval(P[rows], vps[k], maps[k])
                lo[rows], hi[rows] = np.minimum(lo[rows], l), np.maximum(hi[rows], h)
    return lo, hi, c_lo, c_hi


# ---- ssao.frag -----------------------------------------------------------------------------------------------------------------
KERNEL = np.array([  # ssao.frag:31-64, kernelSamples[i].xyz
    (-0.68217, 0.23565, 0.48243), (-0.14448, 0.01628, 0.22807), (0.00604, 0.01909, 0.0127), (0.09733, 0.39072, 0.7324),
    (0.06055, 0.87847, 0.33303), (0.00734, 0.19034, 0.13091), (-0.01377, 0.01745, 0.00399), (0.01468, 0.16627, 0.09108),
    (-0.10093, -0.08015, 0.06625), (-0.27125, -0.39937, 0.0601), (-0.06181, -0.03065, 0.01213), (-0.40189, -0.48095, 0.21808),
    (0.04027, -0.05818, 0.26542), (-0.33535, -0.07516, 0.24997), (0.32748, -0.18112, 0.27292), (0.53962, -0.03361, 0.58926),
    (-0.09598, -0.25424, 0.35754), (-0.17368, 0.01261, 0.23964), (0.1283, 0.12573, 0.16467), (-0.34418, 0.19403, 0.70285),
    (-0.09686, -0.0928, 0.11447), (0.32727, -0.49713, 0.17518), (0.12345, 0.13862, 0.23822), (-0.39258, -0.31128, 0.67374),
    (0.03308, 0.07616, 0.03422), (-0.31777, 0.1885, 0.40808), (-0.17464, 0.28096, 0.11686), (-0.50199, -0.49002, 0.2709),
    (0.38629, 0.15627, 0.56716), (0.06649, -0.05762, 0.0857), (-0.1065, -0.11726, 0.10818), (0.53236, -0.5286, 0.45444)], F).astype(D)
# A sample whose depth comparison is closer than this (relative to the view-space depths involved) may go either way in float32: the
# view transform, the TBN basis and the projection each round a few times, and the bilinear position read moves with the rounding of
# its texel coordinate (SSAO_DXY texels, evaluated at the four corners of that box).
SSAO_EPS = 2.0 ** -16
SSAO_DXY = 2.0 ** -12


def _mat(m):
    return np.array(m[:], D).reshape(4, 4).T  # column-major uniform -> row-major matrix


def ssao(position, normal, view, rows=None):
    """ssao.frag in float64 with an interval: (lo, hi) uint16 images (len(rows) or H, W) that must hold the device's SSAO texels. Texel
    (x, y) is the occlusion of G-buffer texel (x, H-1-y); rows selects SSAO texel rows"""
    H, W = position.shape[:2]
    rows = np.arange(H) if rows is None else np.asarray(rows)
    src = position[H - 1 - rows]
    p = src[..., :3].reshape(-1, 3).astype(D)
    nw = normal[H - 1 - rows][..., :3].reshape(-1, 3).astype(D)
    Vm, Pm, IV = _mat(view.view), _mat(view.projection), _mat(view.inverse_view)
    sky = (src[..., 0] == 1) & (src[..., 1] == 1) & (src[..., 2] == 1)
    sky = sky.reshape(-1)
    with np.errstate(all="ignore"):
        frag = p @ Vm[:3, :3].T + Vm[:3, 3]                                # frag:73
        nv = normalize(nw @ IV.T[:3, :3].T)                               # frag:81-83: transpose(inverse(view)) (n, 0)
        r = np.array([1.0, 1.0, 0.0])
        tangent = normalize(r[None, :] - nv * dot(r[None, :], nv)[:, None])
        bitangent = np.cross(tangent, nv)
        lo, hi = np.zeros(len(p)), np.zeros(len(p))
        radius = c(0.1)
        for kx, ky, kz in KERNEL:
            sp = frag + (tangent * kx + bitangent * ky + nv * kz) * radius  # frag:98-99
            cl = sp @ Pm[:, :3].T + Pm[:, 3]
            u = (cl[:, 0] / cl[:, 3]) * 0.5 + 0.5
            v = 1.0 - ((cl[:, 1] / cl[:, 3]) * 0.5 + 0.5)                  # FLIP_UV_Y
            x, y = u * W - 0.5, v * H - 0.5
            depths = [(bilinear(position[..., :3], x + dx, y + dy) @ Vm[2, :3] + Vm[2, 3]) for dx in (-SSAO_DXY, SSAO_DXY) for dy in (-SSAO_DXY, SSAO_DXY)]
            depths.append(bilinear(position[..., :3], x, y) @ Vm[2, :3] + Vm[2, 3])
            dmin, dmax = np.min(depths, axis=0), np.max(depths, axis=0)
            eps = SSAO_EPS * (np.abs(frag[:, 2]) + np.abs(sp[:, 2]) + np.abs(dmax) + np.abs(dmin) + radius)
            dmin, dmax = dmin - eps, dmax + eps
            # smoothstep(0, 1, radius / |frag.z - depth|) over the depth interval: its extremes at the interval's ends, 1 if it holds frag.z
            rng = lambda dd: (lambda t: t * t * (3.0 - 2.0 * t))(np.clip(radius / np.abs(frag[:, 2] - dd), 0.0, 1.0))
            r_a, r_b = rng(dmin), rng(dmax)
            inside = (dmin <= frag[:, 2]) & (frag[:, 2] <= dmax)
            r_lo, r_hi = np.minimum(r_a, r_b), np.where(inside, 1.0, np.maximum(r_a, r_b))
            surely, maybe = dmin >= sp[:, 2], dmax >= sp[:, 2]                # frag:111: sampleDepth >= samplePos.z
            lo = lo + np.where(surely, r_lo, 0.0)
            hi = hi + np.where(maybe, r_hi, 0.0)
        occ_lo = 1.0 - (hi / 32.0) * c(1.6)                               # frag:114-115
        occ_hi = 1.0 - (lo / 32.0) * c(1.6)
        occ_lo, occ_hi = np.where(sky, 1.0, occ_lo), np.where(sky, 1.0, occ_hi)
    # the float32 sum of 32 terms and the final scale: 2^-18 of the result, far below half a step of 65535
    q_lo = np.ceil(np.clip(occ_lo, 0.0, 1.0) * 65535.0 - 0.5 - 1e-3)
    q_hi = np.floor(np.clip(occ_hi, 0.0, 1.0) * 65535.0 + 0.5 + 1e-3)
    shape = (len(rows), W)
    return q_lo.reshape(shape).astype(np.int64), q_hi.reshape(shape).astype(np.int64)


# ---- present.frag (FXAA off) ---------------------------------------------------------------------------------------------------
def linear_to_srgb(x):
    """view.glsl:53-61 in float64"""
    x = np.asarray(x, D)
    with np.errstate(all="ignore"):
        return np.where(x < c(0.0031308), x * c(12.92), c(1.055) * np.power(np.where(x < 0, 0.0, x), c(1.0) / c(2.4)) - c(0.055))


def present(img):
    """present.frag with fxaa_enabled = 0: texture(in_color_texture, FLIP_UV_Y(in_uv)) then linearToSrgb, stored B, G, R as
    round(clamp(x) 255) with NaN as 0, alpha 255. Returns (H, W, 4) float64 before rounding (B, G, R, 255) and the uint8 image"""
    H, W = img.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    u, v = (x.reshape(-1) + 0.5) / W, (y.reshape(-1) + 0.5) / H
    color = bilinear(img[..., :3], u * W - 0.5, v * H - 0.5)
    s = np.nan_to_num(np.clip(linear_to_srgb(color), 0.0, 1.0), nan=0.0) * 255.0
    out = np.full((H * W, 4), 255.0)
    out[:, 0], out[:, 1], out[:, 2] = s[:, 2], s[:, 1], s[:, 0]
    return out.reshape(H, W, 4), np.rint(out).astype(np.uint8).reshape(H, W, 4)

"""CPU reference of the IBL maps (uh_render_hybrid's UH_HYBRID_ENVIRONMENT: setup_cubemap_pass, ibl.rs) and of their three consumers
(imageBasedLighting in the deferred pass and in rt_reflections' hit shader, the sky's cube lookup), in numpy float32 in the order
DESIGN.md section 2 "Environment and IBL maps" pins, line by line. Built on tests/hybrid_reference.py, tests/hybrid_frame_reference.py
and the oracle's sky and primary_ray. Each filter takes the maps it reads as arguments, so a test can feed it the device's own maps.
Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa

F = np.float32
PI = F(3.14159265359)  # brdf.glsl:1 and the shaders' #define PI round to the same float
SIZE, MIPS, LUT = 512, 8, 512

# face layer f: the unnormalised direction of ndc (x, y) - inverse(look_at_rh(0, f, up)) * (x, y, -1, 0), exact
FACE_DIR = [
    lambda x, y: (np.ones_like(x), -y, -x),   # look_at_rh(0, +X, -Y)
    lambda x, y: (-np.ones_like(x), -y, x),   # (0, -X, -Y)
    lambda x, y: (x, -np.ones_like(x), -y),   # (0, -Y, -Z)
    lambda x, y: (x, np.ones_like(x), y),     # (0, +Y, +Z)
    lambda x, y: (x, -y, np.ones_like(x)),    # (0, +Z, -Y)
    lambda x, y: (-x, -y, -np.ones_like(x)),  # (0, -Z, -Y)
]
# Vulkan's face table: (major axis, sc axis, tc axis, their signs)
FACE_AXES = [(0, 2, 1, 1, -1, -1), (0, 2, 1, -1, 1, -1), (1, 0, 2, 1, 1, 1), (1, 0, 2, -1, 1, -1), (2, 0, 1, 1, 1, -1), (2, 0, 1, -1, -1, -1)]


# ---- glam's matrices, for the closed form's known-answer test ----------------------------------------------------------------------
def glam_look_at_rh(center, up):
    """Mat4::look_at_rh(0, center, up), column-major float32 (16,)"""
    f = np.asarray(center, np.float32)
    f = f / np.float32(np.sqrt(np.dot(f, f)))
    s = np.cross(f, np.asarray(up, np.float32)).astype(np.float32)
    s = s / np.float32(np.sqrt(np.dot(s, s)))
    u = np.cross(s, f).astype(np.float32)
    return np.array([s[0], u[0], -f[0], 0, s[1], u[1], -f[1], 0, s[2], u[2], -f[2], 0, 0, 0, 0, 1], np.float32)


def glam_perspective_rh(fov_deg=90.0, aspect=1.0, near=0.01, far=20000.0):
    fov = F(F(fov_deg) * F(np.pi) / F(180.0))
    h = np.cos(F(0.5) * fov) / np.sin(F(0.5) * fov)
    w = h / F(aspect)
    r = F(far) / (F(near) - F(far))
    return np.array([w, 0, 0, 0, 0, h, 0, 0, 0, 0, r, -1, 0, 0, r * F(near), 0], np.float32)


VIEWS = [((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, -1, 0)), ((0, -1, 0), (0, 0, -1)), ((0, 1, 0), (0, 0, 1)), ((0, 0, 1), (0, -1, 0)), ((0, 0, -1), (0, -1, 0))]


# ---- texel directions, cube addressing, filtering ---------------------------------------------------------------------------------
def texel_uv(i, j, S):
    """in_uv of texel (i, j) of a face of size S under the Y-flipped viewport"""
    i, j = np.asarray(i).astype(np.float32), np.asarray(j).astype(np.float32)
    return (i + F(0.5)) / F(S), F(1.0) - (j + F(0.5)) / F(S)


def texel_dir(f, i, j, S):
    """world_dir_from_uv at texel (i, j) of face f (scalar), size S: (N, 3) float32, normalised"""
    u, v = texel_uv(i, j, S)
    x, y = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    return hr.normalize(np.stack([np.asarray(c, np.float32) for c in FACE_DIR[f](x, y)], axis=-1))


def cube_coords(d):
    """face, s, t of directions d (N, 3): ties to x, then y; a zero major component counts as positive; s = (sc * (1 / ma)) * 0.5 + 0.5"""
    d = np.asarray(d, np.float32)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    px, py, pz = ~(d[:, 0] < 0), ~(d[:, 1] < 0), ~(d[:, 2] < 0)
    face = np.where(isx, np.where(px, 0, 1), np.where(isy, np.where(py, 2, 3), np.where(pz, 4, 5)))
    ma = np.where(isx, ax, np.where(isy, ay, az))
    sc = np.where(isx, np.where(px, -d[:, 2], d[:, 2]), np.where(isy, d[:, 0], np.where(pz, d[:, 0], -d[:, 0])))
    tc = np.where(isx, -d[:, 1], np.where(isy, np.where(py, d[:, 2], -d[:, 2]), -d[:, 1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / ma
        return face, (sc * inv) * F(0.5) + F(0.5), (tc * inv) * F(0.5) + F(0.5)


def folded_texel(f, i, j, S):
    """(face, i, j) -> flat index face * S^2 + j * S + i; i or j (not both) may be -1 or S: folded across that edge onto the neighbour"""
    f, i, j = np.broadcast_arrays(np.asarray(f, np.int64), np.asarray(i, np.int64), np.asarray(j, np.int64))
    out = np.empty(f.shape, np.int64)
    for face in range(6):
        sel = f == face
        if not sel.any():
            continue
        ma, sc, tc, ms, ss, ts = FACE_AXES[face]
        a, b = 2 * i[sel] + 1 - S, 2 * j[sel] + 1 - S
        P = np.zeros((3, a.size), np.int64)
        P[ma], P[sc], P[tc] = ms * S, ss * a, ts * b
        axis = np.full(a.size, ma)
        oa_, ob = (a < -S) | (a > S), ~((a < -S) | (a > S)) & ((b < -S) | (b > S))
        P[ma] = np.where(oa_ | ob, ms * (S - 1), P[ma])
        P[sc] = np.where(oa_, ss * np.where(a < 0, -S, S), P[sc])
        P[tc] = np.where(ob, ts * np.where(b < 0, -S, S), P[tc])
        axis = np.where(oa_, sc, np.where(ob, tc, axis))
        pa = P[axis, np.arange(a.size)]
        nf = 2 * axis + (pa < 0)
        res = np.empty(a.size, np.int64)
        for g in range(6):
            sg = nf == g
            _, gsc, gtc, _, gss, gts = FACE_AXES[g]
            na, nb = gss * P[gsc, sg], gts * P[gtc, sg]
            res[sg] = g * S * S + ((nb + S - 1) // 2) * S + (na + S - 1) // 2
        out[sel] = res
    return out


def edge_texel(flat, f, i, j, S):
    """the texel at (i, j) in [-1, S]^2 of face f from a level flattened to (6 S^2, 3+); corners: ((own + across i) + across j) * (1 / 3)"""
    corner = ((i < 0) | (i >= S)) & ((j < 0) | (j >= S))
    out = np.empty((len(f), 3), np.float32)
    nc = ~corner
    out[nc] = flat[folded_texel(f[nc], i[nc], j[nc], S), :3]
    if corner.any():
        fc, ic, jc = f[corner], i[corner], j[corner]
        ci, cj = np.where(ic < 0, 0, S - 1), np.where(jc < 0, 0, S - 1)
        own = flat[fc * S * S + cj * S + ci, :3]
        out[corner] = ((own + flat[folded_texel(fc, ic, cj, S), :3]) + flat[folded_texel(fc, ci, jc, S), :3]) * F(1.0 / 3.0)
    return out


def cube_bilinear(level, d):
    """texture(cube, d) at one level (6, S, S, 4) through LINEAR, seamless: (N, 3)"""
    S = level.shape[1]
    flat = level.reshape(6 * S * S, -1)
    f, s, t = cube_coords(d)
    x, y = s * F(S) - F(0.5), t * F(S) - F(0.5)
    ok = (x >= -1) & (x < S) & (y >= -1) & (y < S)
    x, y = np.where(ok, x, F(0.0)), np.where(ok, y, F(0.0))
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[:, None], (y - fy)[:, None]
    i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
    inner = (i0 >= 0) & (j0 >= 0) & (i0 + 1 < S) & (j0 + 1 < S)
    t00, t10, t01, t11 = (np.empty((len(f), 3), np.float32) for _ in range(4))
    base = f * S * S + j0 * S + i0
    for arr, di, dj in ((t00, 0, 0), (t10, 1, 0), (t01, 0, 1), (t11, 1, 1)):
        arr[inner] = flat[base[inner] + dj * S + di, :3]
        e = ~inner
        if e.any():
            arr[e] = edge_texel(flat, f[e], i0[e] + di, j0[e] + dj, S)
    a = t00 * (F(1.0) - ax) + t10 * ax
    b = t01 * (F(1.0) - ax) + t11 * ax
    return np.where(ok[:, None], a * (F(1.0) - ay) + b * ay, F(0.0))


def cube_lod(levels, d, lod):
    """textureLod(cube, d, lod), levels a list of (6, S, S, 4) arrays (mip 0 first): trilinear between floor and floor + 1 of the clamped lod"""
    lod = np.minimum(np.maximum(np.broadcast_to(np.asarray(lod, np.float32), (len(d),)), F(0.0)), F(len(levels) - 1))
    fl = np.floor(lod)
    m0 = fl.astype(np.int64)
    m1 = np.minimum(m0 + 1, len(levels) - 1)
    fr_ = (lod - fl)[:, None]
    c0, c1 = np.empty((len(d), 3), np.float32), np.empty((len(d), 3), np.float32)
    for m in np.unique(m0):
        sel = m0 == m
        c0[sel] = cube_bilinear(levels[m], d[sel])
    c1[:] = c0
    need = fr_[:, 0] != 0
    for m in np.unique(m1[need]):
        sel = need & (m1 == m)
        c1[sel] = cube_bilinear(levels[m], d[sel])
    return c0 * (F(1.0) - fr_) + c1 * fr_


def lut_bilinear(lut, u, v):
    """the BRDF LUT (512, 512, 2) float16 through LINEAR + MIRRORED_REPEAT at uv: (N, 2)"""
    img = np.zeros(lut.shape[:2] + (3,), np.float32)
    img[..., :2] = lut.astype(np.float32)
    return fr.bilinear(img, u * F(LUT) - F(0.5), v * F(LUT) - F(0.5))[:, :2]


# ---- brdf.glsl --------------------------------------------------------------------------------------------------------------------
def random2(cx, cy, sin_ulps=0):
    """random(co): mod(x, y) = x - y * floor(x / y); numpy's float32 sin where the device uses sinf. sin_ulps moves the sine by that many
    float32 ulps (the device's sinf may round the other way)"""
    dt = np.asarray(cx, np.float32) * F(12.9898) + np.asarray(cy, np.float32) * F(78.233)
    sn = dt - F(3.14) * np.floor(dt / F(3.14))
    s = np.sin(sn).astype(np.float32)
    for _ in range(abs(sin_ulps)):
        s = np.nextafter(s, F(np.inf) if sin_ulps > 0 else F(-np.inf)).astype(np.float32)
    r = s * F(43758.5453)
    return r - np.floor(r)


def hammersley2d(i, N):
    bits = np.asarray(i, np.uint32)
    bits = (bits << np.uint32(16)) | (bits >> np.uint32(16))
    for m, s in ((0x55555555, 1), (0x33333333, 2), (0x0F0F0F0F, 4), (0x00FF00FF, 8)):
        m, n, s = np.uint32(m), np.uint32(~m & 0xFFFFFFFF), np.uint32(s)
        bits = ((bits & m) << s) | ((bits & n) >> s)
    return np.asarray(i, np.uint32).astype(np.float32) / F(N), bits.astype(np.float32) * F(2.3283064365386963e-10)


def importance_sample_ggx(xi_x, xi_y, roughness, N, rnd):
    """importanceSample_GGX, vectorised over (N, 3) normals with their random(normal.xz)"""
    alpha = roughness * roughness
    phi = (F(2.0) * PI) * xi_x + rnd * F(0.1)
    cos_t = np.sqrt((F(1.0) - xi_y) / (F(1.0) + (alpha * alpha - F(1.0)) * xi_y))
    sin_t = np.sqrt(F(1.0) - cos_t * cos_t)
    H = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), np.broadcast_to(cos_t, phi.shape)], axis=-1).astype(np.float32)
    up = np.where((np.abs(N[:, 2]) < F(0.999))[:, None], np.array([0, 0, 1], np.float32), np.array([1, 0, 0], np.float32))
    tx = hr.normalize(hr.cross(up, N))
    ty = hr.normalize(hr.cross(N, tx))
    return hr.normalize((tx * H[:, 0:1] + ty * H[:, 1:2]) + N * H[:, 2:3])


# ---- the four maps ------------------------------------------------------------------------------------------------------------------
def environment(eye, sun, f, i, j, S):
    """cubemap.frag at texels (i, j) of face f, size S, through the oracle's sky (which normalises the sun: pass a unit sun)"""
    d = texel_dir(f, i, j, S)
    return np.array([oa.sky(eye, dd, sun) for dd in d], np.float32)


def irradiance_taps():
    """irradiance_filter.frag's loops: (15876, 4) = (sin t cos p, sin t sin p, cos t, sin t), phi-major; sin / cos in double, rounded"""
    taps = []
    phi = F(0.0)
    while phi < F(2.0) * PI:
        theta = F(0.0)
        while theta < F(0.5) * PI:
            st, ct = F(np.sin(np.float64(theta))), F(np.cos(np.float64(theta)))
            cp, sp = F(np.cos(np.float64(phi))), F(np.sin(np.float64(phi)))
            taps.append((st * cp, st * sp, ct, st))
            theta = F(theta + F(0.025))
        phi = F(phi + F(0.025))
    return np.array(taps, np.float32)


def irradiance(env0, f, i, j, taps=None):
    """irradiance_filter.frag at texels (i, j) of face f on environment mip 0 (6, 512, 512, 4), the taps summed in order: (N, 3)"""
    taps = irradiance_taps() if taps is None else taps
    N = texel_dir(f, i, j, SIZE)
    up0 = np.broadcast_to(np.array([0, 1, 0], np.float32), N.shape)
    right = hr.normalize(hr.cross(up0, N))
    up = hr.normalize(hr.cross(N, right))
    acc = np.zeros((len(N), 3), np.float32)
    for k0 in range(0, len(taps), 2048):
        tp = taps[k0 : k0 + 2048]
        sv = (right[None] * tp[:, None, 0:1] + up[None] * tp[:, None, 1:2]) + N[None] * tp[:, None, 2:3]
        c = cube_bilinear(env0, sv.reshape(-1, 3)).reshape(len(tp), len(N), 3)
        c = (c * tp[:, None, 2:3]) * tp[:, None, 3:4]
        for k in range(len(tp)):
            acc = acc + c[k]
    return (PI * acc) * (F(1.0) / F(len(taps)))


def specular(env_levels, m, f, i, j, sin_ulps=0):
    """specular_filter.frag (prefilterEnvMap(N, m / 7), envMapDim 512) at texels (i, j) of face f of mip m: (N, 3); sin_ulps: random2's"""
    rough = F(m) / F(MIPS - 1)
    N = texel_dir(f, i, j, SIZE >> m)
    V = N
    rnd = random2(N[:, 0], N[:, 2], sin_ulps)
    alpha = rough * rough
    alpha2 = alpha * alpha
    dim = F(SIZE)
    omega_p = (F(4.0) * PI) / ((F(6.0) * dim) * dim)
    color, total = np.zeros((len(N), 3), np.float32), np.zeros(len(N), np.float32)
    with np.errstate(all="ignore"):
        for s in range(32):
            xx, xy = hammersley2d(s, 32)
            H = importance_sample_ggx(np.full(len(N), xx, np.float32), np.full(len(N), xy, np.float32), rough, N, rnd)
            L = H * (F(2.0) * hr.dot(V, H))[:, None] - V
            nl = np.minimum(np.maximum(hr.dot(N, L), F(0.0)), F(1.0))
            nh = np.minimum(np.maximum(hr.dot(N, H), F(0.0)), F(1.0))
            vh = np.minimum(np.maximum(hr.dot(V, H), F(0.0)), F(1.0))
            den = (nh * nh) * (alpha2 - F(1.0)) + F(1.0)
            D = alpha2 / ((PI * den) * den)
            pdf = (D * nh) / (F(4.0) * vh) + F(0.0001)
            omega_s = F(1.0) / (F(32.0) * pdf)
            lod = np.zeros(len(N), np.float32) if rough == 0 else np.maximum(F(0.5) * np.log2(omega_s / omega_p) + F(1.0), F(0.0))
            use = nl > 0
            if use.any():
                c = cube_lod(env_levels, L[use], lod[use])
                color[use] = color[use] + c * nl[use][:, None]
                total[use] = total[use] + nl[use]
        return color / total[:, None]


def brdf_lut(rows=None):
    """brdf_lut.frag: (len(rows), 512, 2) float32 before the fp16 store; texel (x, y) at NoV = (x + 0.5) / 512, roughness = 1 - (y + 0.5) / 512"""
    rows = np.arange(LUT) if rows is None else np.asarray(rows)
    rough = (F(1.0) - (rows.astype(np.float32) + F(0.5)) / F(LUT))[:, None]           # (R, 1)
    NoV = ((np.arange(LUT, dtype=np.float32) + F(0.5)) / F(LUT))[None, :]               # (1, X)
    Vx, Vz = np.sqrt(F(1.0) - NoV * NoV), NoV
    a2 = np.power(rough, F(4.0))
    oma2 = F(1.0) - a2
    ggxl_v = (NoV * NoV) * oma2 + a2
    rnd = random2(F(0.0), F(1.0))
    Nz = np.tile(np.array([[0, 0, 1]], np.float32), (len(rows), 1))
    A = np.zeros((len(rows), LUT), np.float32)
    B = np.zeros((len(rows), LUT), np.float32)
    with np.errstate(all="ignore"):
        for k in range(1024):
            xx, xy = hammersley2d(k, 1024)
            H = importance_sample_ggx(np.full(len(rows), xx, np.float32), np.full(len(rows), xy, np.float32), rough[:, 0], Nz, np.full(len(rows), rnd, np.float32))
            Hx, Hy, Hz = H[:, 0:1], H[:, 1:2], H[:, 2:3]
            vdh = (Vx * Hx + F(0.0) * Hy) + Vz * Hz
            Lx, Ly, Lz = Hx * (F(2.0) * vdh) - Vx, Hy * (F(2.0) * vdh) - F(0.0), Hz * (F(2.0) * vdh) - Vz
            NoL = np.minimum(np.maximum((F(0.0) * Lx + F(0.0) * Ly) + F(1.0) * Lz, F(0.0)), F(1.0))
            NoH = np.minimum(np.maximum((F(0.0) * Hx + F(0.0) * Hy) + F(1.0) * Hz, F(0.0)), F(1.0))
            VoH = np.minimum(np.maximum(vdh, F(0.0)), F(1.0))
            ggxv = NoL * np.sqrt(ggxl_v)
            ggxl = NoV * np.sqrt((NoL * NoL) * oma2 + a2)
            vis = F(0.5) / (ggxv + ggxl)
            v_pdf = ((vis * VoH) * NoL) / NoH
            fc = np.power(F(1.0) - VoH, F(5.0))
            use = NoL > 0
            A = np.where(use, A + (F(1.0) - fc) * v_pdf, A)
            B = np.where(use, B + fc * v_pdf, B)
    return np.stack([(F(4.0) * A) / F(1024.0), (F(4.0) * B) / F(1024.0)], axis=-1)


# ---- the consumers ----------------------------------------------------------------------------------------------------------------
def image_based_lighting(maps, P, base, N, metallic, roughness, occlusion, eye):
    """pbr_lighting.glsl:81-108 on maps = dict(irr=(6,512,512,4), spec=[8 levels], lut=(512,512,2) float16): (N, 3)"""
    with np.errstate(all="ignore"):
        V = hr.normalize(np.asarray(eye, np.float32)[None, :] - P)
        R = -(V - N * (F(2.0) * hr.dot(N, V))[:, None])
        om = F(1.0) - metallic
        F0 = np.full((len(P), 3), F(0.04), np.float32) * om[:, None] + base * metallic[:, None]
        NdotV = np.maximum(hr.dot(N, V), F(0.0))
        x = np.minimum(np.maximum(F(1.0) - NdotV, F(0.0)), F(1.0))
        p5 = ((x * x) * (x * x)) * x
        omr = F(1.0) - roughness
        Fr = F0 + (np.maximum(omr[:, None], F0) - F0) * p5[:, None]
        kD = (F(1.0) - Fr) * om[:, None]
        irr = cube_bilinear(maps["irr"], N)
        diffuse = irr * base
        pre = cube_lod(maps["spec"], R, roughness * F(7.0))
        brdf = lut_bilinear(maps["lut"], NdotV, F(1.0) - roughness)
        specular = pre * (Fr * brdf[:, 0:1] + brdf[:, 1:2])
        return (kD * diffuse + specular) * occlusion[:, None]


def read_maps(r):
    """the device's four maps as the consumers read them"""
    return dict(env=[np.stack([r.read_environment(0, f, m) for f in range(6)]) for m in range(MIPS)],
                irr=np.stack([r.read_environment(1, f, 0) for f in range(6)]),
                spec=[np.stack([r.read_environment(2, f, m) for f in range(6)]) for m in range(MIPS)],
                lut=r.read_environment(3))


def _view_copy(view, **kw):
    v = type(view).from_buffer_copy(view)
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def deferred_ibl(g, shadows, reflections, ssao_img, view, meshes, lights, maps):
    """deferred.frag with ibl_enabled = 1: the direct light Lo of hybrid_frame_reference.deferred (occlusion 0 there leaves Lo alone),
    plus imageBasedLighting, then the reflections / shadows / SSAO steps of that function"""
    H, W = g["position"].shape[:2]
    g0 = dict(g)
    g0["pbr"] = g["pbr"].copy()
    g0["pbr"][..., 2] = 0.0
    Lo = fr.deferred(g0, shadows, reflections, ssao_img, _view_copy(view, raytracing_supported=0, ssao_enabled=0), meshes, lights)[..., :3].reshape(-1, 3)
    P, N, R = g["position"][..., :3].reshape(-1, 3), g["normal"][..., :3].reshape(-1, 3), g["pbr"].reshape(-1, 4)
    material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    table = lambda key, default: np.where(valid, np.array([m[key] for m in meshes] or [default], np.float32)[idx], F(default))
    mf, rf, typ = table("metallic", 1.0), table("roughness", 1.0), table("type", 0.0)
    bc = np.where(valid[:, None], np.array([m["base_color"] for m in meshes] or [np.ones(3)], np.float32)[idx], F(1.0))
    base = fr.gamma_table()[g["albedo"].reshape(-1, 4)[:, :3]] * bc
    amb = image_based_lighting(maps, P, base, N, R[:, 0] * mf, R[:, 1] * rf, R[:, 2], view.eye_pos[:])
    with np.errstate(all="ignore"):
        color = amb + Lo
        if view.raytracing_supported == 1:
            refl = fr.unorm_lut(reflections.reshape(-1, 4)[:, :3])
            color = np.where((typ == 1.0)[:, None], color * (F(1.0) - F(1.0)) + refl * F(1.0), color)
            color = color * np.maximum(fr.unorm_lut(shadows.reshape(-1)), F(0.3))[:, None]
        if view.ssao_enabled == 1:
            color = color * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
    out = np.ones((H * W, 4), np.float32)
    out[:, :3] = color
    return out.reshape(H, W, 4)


def sky_cube(position, view, env_levels):
    """atmosphere.frag with cubemap_enabled = 1 on the G-buffer's miss pixels: {(y, x): rgb} = textureLod(env, dir * (1, -1, 1), 2)"""
    H, W = position.shape[:2]
    keys = [(int(y), int(x)) for y, x in zip(*np.nonzero(position[..., 3] == 0))]
    if not keys:
        return {}
    d = np.array([oa.primary_ray(view, W, H, x, y, 0.5, 0.5)[3:] for y, x in keys], np.float32)
    d[:, 1] = -d[:, 1]
    c = cube_lod(env_levels, d, np.full(len(d), 2.0, np.float32))
    return dict(zip(keys, c))


def reflections_ibl(oracle, meshes, position, normal, pbr, view, maps):
    """rt_reflections with ibl_enabled = 1: hybrid_reference.reflections, with the hit pixels shaded by imageBasedLighting (rchit:50-61)"""
    out, kind = hr.reflections(oracle, meshes, position, normal, pbr, view)
    H, W = position.shape[:2]
    p, n = hr.corner(position)[..., :3].reshape(-1, 3), hr.corner(normal)[..., :3].reshape(-1, 3)
    idx = np.nonzero(kind.reshape(-1) == 1)[0]
    if not idx.size:
        return out, kind
    o = hr.offset_ray(p[idx], n[idx])
    eye = np.array(view.eye_pos[:], dtype=np.float32)
    I = -hr.normalize(eye[None, :] - o)
    d = I - n[idx] * (F(2.0) * hr.dot(n[idx], I))[:, None]
    t, u, v, mesh, prim = hr.trace(oracle, o, d)
    b0, b1, b2 = (F(1.0) - u) - v, u, v
    uu, vv = hr._uv(meshes, mesh, prim, b0, b1, b2)
    nrm = np.zeros((len(idx), 3), np.float32)
    for m in np.unique(mesh):
        sel = mesh == m
        M = meshes[int(m)]
        tri = M["indices"].reshape(-1, 3)[prim[sel]]
        vn = [M["vertices"]["normal"][tri[:, k], :3].astype(np.float32) for k in range(3)]
        nn = (vn[0] * b0[sel][:, None] + vn[1] * b1[sel][:, None]) + vn[2] * b2[sel][:, None]
        nrm[sel] = hr.normalize(hr.inverse_transpose_mul(hr.invert3x3(M["world"]), nn))
    nrm = np.where((hr.dot(nrm, d) > 0)[:, None], -nrm, nrm)
    tex = lambda key: hr.sample(oracle, np.array([meshes[int(m)][key] for m in mesh], np.uint32), uu, vv)
    base = tex("diffuse_map") * np.array([meshes[int(m)]["base_color"] for m in mesh], np.float32).reshape(-1, 3)
    mr, oc = tex("metallic_roughness_map"), tex("occlusion_map")
    pos = o + t[:, None] * d
    c = image_based_lighting(maps, pos, base, nrm, mr[:, 2], mr[:, 1], oc[:, 0], eye)
    flat = out.reshape(-1, 4)
    flat[idx, :3] = hr.unorm8(c)
    return flat.reshape(H, W, 4), kind

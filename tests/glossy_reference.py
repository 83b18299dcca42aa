"""CPU restatement of the ray-traced glossy reflections (uh_render_hybrid's UH_HYBRID_GLOSSY): which pixels cast, their rays drawn from the
GGX distribution of visible normals, the weight of each ray, its radiance (the rtgi pass's), the ray counts, the per-pixel split sums in
sample order, the roughness-aware filter and the composite into deferred_output, in numpy float32 in the order DESIGN.md section 2
"Ray-traced glossy reflections" pins. Composed from tests/rtgi_reference.py (rays: the radiance of a ray, with this pass's directions in
place of its own; clamp, _shifted, the scenes), tests/rtao_reference.py (normals), tests/hybrid_reference.py (dot, normalize, cross,
offset_ray) and tests/hybrid_frame_reference.py (gamma_table), and the oracle's init_rng, random_point_in_unit_disk and frame_number. Each
function takes the G-buffer as an argument, so a test can feed it the device's own. With the scenes the tests use.
Not a conftest: test modules import it."""
import functools

import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao
import rtgi_reference as gi

F = np.float32
SEED_XOR = 0x474C4F53
SUNLIT, DARK, EMITTER, MISSED = gi.SUNLIT, gi.DARK, gi.EMITTER, gi.MISSED
W, H = gi.W, gi.H


def default_params(**kw):
    """uh_glossy_default_params, with `kw` over it"""
    p = dict(samples=1, blur_radius=3, max_roughness=0.6, max_radiance=16.0, intensity=1.0, blur_roughness=0.5, blur_normal_cos=0.95, blur_plane=0.05)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def pos(x):
    """x > 0 ? x : 0: a NaN, a negative and -0 become +0"""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, F(0.0)).astype(np.float32)


def material_table(g, meshes):
    """per pixel (flattened), as k_hybrid_deferred forms the record: metallic, roughness factors and type (1, 1, 0 out of range), base colour"""
    R = g["pbr"].reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    table = lambda key, default: np.where(valid, np.array([m[key] for m in meshes] or [default], np.float32)[idx], F(default))
    bc = np.where(valid[:, None], np.array([m["base_color"] for m in meshes] or [np.ones(3)], np.float32)[idx], F(1.0))
    return table("metallic", 1.0), table("roughness", 1.0), table("type", 0.0), bc


def pixels(g, view, meshes, params):
    """the pixels that cast: dict(rows (m,) into the flattened frame, P, Nn, V (m, 3), NoV, r (m,), re (m,) int) and, over the whole frame
    (flattened), why a pixel that passes RTGI's rule does not cast: metal, rough"""
    Nn, geo = ao.normals(g)
    _, rf, typ, _ = material_table(g, meshes)
    P = g["position"][..., :3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        metal = geo & (view.raytracing_supported == 1) & (typ == 1.0)
        r = g["pbr"].reshape(-1, 4)[:, 1] * rf
        in_window = (r >= 0) & (r <= F(params["max_roughness"]))
        rough = geo & ~metal & ~in_window
        V = hr.normalize(np.array(view.eye_pos[:3], np.float32)[None, :] - P)
        NoV = hr.dot(Nn, V)
        cast = geo & ~metal & in_window & np.isfinite(V).all(axis=1) & (NoV > 0)
        rows = np.nonzero(cast)[0]
        re = (np.minimum(r[rows] / F(params["blur_roughness"]), F(1.0)) * F(params["blur_radius"])).astype(np.int32)
    return dict(rows=rows, P=P[rows], Nn=Nn[rows], V=V[rows], NoV=NoV[rows], r=r[rows], re=re, metal=metal, rough=rough)


@functools.lru_cache(maxsize=None)
def _disk_points(Ww, Hh, word):
    """randomPointInUnitDisk of the state initRNG(px, py, W, word) for every pixel of a W x H frame: (H * W, 2)"""
    out = np.empty((Ww * Hh, 2), np.float32)
    for pix in range(Ww * Hh):
        out[pix], _ = oa.random_point_in_unit_disk(oa.init_rng(pix % Ww, pix // Ww, Ww, word))
    out.setflags(write=False)
    return out


def frame(n):
    """T, B of Nn (.., 3): Duff et al. 2017"""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    sign = np.copysign(F(1.0), z)
    a = F(-1.0) / (sign + z)
    b = (x * y) * a
    T = np.stack([F(1.0) + ((sign * x) * x) * a, sign * b, -(sign * x)], axis=-1)
    B = np.stack([b, sign + (y * y) * a, -y], axis=-1)
    return T, B


def sample(Nn, V, NoV, r, t):
    """one sample of each of m pixels from its disk point t (m, 2): dict(Hw, d (m, 3), NoL, VoH, Gw, x5 (m,), below (m,))"""
    with np.errstate(all="ignore"):
        alpha = r * r
        a2 = alpha * alpha
        T, B = frame(Nn)
        Ve = np.stack([hr.dot(V, T), hr.dot(V, B), NoV], axis=-1)
        Vh = hr.normalize(np.stack([alpha * Ve[:, 0], alpha * Ve[:, 1], Ve[:, 2]], axis=-1))
        lensq = Vh[:, 0] * Vh[:, 0] + Vh[:, 1] * Vh[:, 1]
        ln = np.sqrt(lensq)
        zero = np.zeros_like(lensq)
        T1 = np.where((lensq > 0)[:, None], np.stack([-Vh[:, 1] / ln, Vh[:, 0] / ln, zero], axis=-1), np.array([1, 0, 0], np.float32)[None, :]).astype(np.float32)
        T2 = hr.cross(Vh, T1)
        t1, t2 = t[:, 0], t[:, 1]
        sh = F(0.5) * (F(1.0) + Vh[:, 2])
        t2 = (F(1.0) - sh) * np.sqrt(F(1.0) - t1 * t1) + sh * t2
        c = np.sqrt(pos((F(1.0) - t1 * t1) - t2 * t2))
        Nh = (t1[:, None] * T1 + t2[:, None] * T2) + c[:, None] * Vh
        Ne = hr.normalize(np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], pos(Nh[:, 2])], axis=-1))
        Hw = (Ne[:, 0:1] * T + Ne[:, 1:2] * B) + Ne[:, 2:3] * Nn
        VoH = hr.dot(V, Hw)
        d = hr.normalize((F(2.0) * VoH)[:, None] * Hw - V)
        NoL = hr.dot(Nn, d)
        below = ~(NoL > 0)
        sv = np.sqrt((NoV * NoV) * (F(1.0) - a2) + a2)
        sl = np.sqrt((NoL * NoL) * (F(1.0) - a2) + a2)
        Gw = (NoL * (NoV + sv)) / (NoL * sv + NoV * sl)
        x = F(1.0) - VoH
        x5 = ((x * x) * (x * x)) * x
    return dict(Hw=Hw.astype(np.float32), d=d.astype(np.float32), NoL=NoL, VoH=VoH, Gw=Gw.astype(np.float32), x5=x5.astype(np.float32), below=below)


def samples(g, view, px, n):
    """the n samples of the pixels px (pixels()): a list of sample() dicts in sample order"""
    Hh, Ww = g["position"].shape[:2]
    frame_no = oa.frame_number(view)
    out = []
    for s in range(n):
        word = ((frame_no * 64 + s) ^ SEED_XOR) & 0xFFFFFFFF
        out.append(sample(px["Nn"], px["V"], px["NoV"], px["r"], _disk_points(Ww, Hh, word)[px["rows"]]))
    return out


def radiance(oracle, meshes, g, view, rows, nn, d, max_radiance, furnace=False):
    """L, kind and the sun-ray count of the rays d (k, 3) cast from the pixels rows (k,), which may repeat: rtgi_reference.rays with every
    ray as the one sample of a pixel of its own, and these directions where it draws its own"""
    saved = gi.directions
    gi.directions = lambda g_, view_, samples_: (rows, nn, d[:, None, :])
    try:
        r = gi.rays(oracle, meshes, g, view, 1, max_radiance, furnace)
    finally:
        gi.directions = saved
    # rtgi_reference.py is left as it is, so the directions enter through its module name; this fails if rays() ever stops looking it up
    assert r["rows"] is rows and r["L"].shape == (len(rows), 1, 3), "rtgi_reference.rays took these rays, one per row"
    return r["L"][:, 0], r["kind"][:, 0], r["shadow_rays"]


def gather(oracle, meshes, g, view, params, furnace=False, order=None):
    """the pass up to its filter: dict(counts (H, W, 4) uint8, S, Bi (H, W, 3) float32 (0 where nothing was cast), cast (H, W), re (H, W)
    int32 (-1 where nothing was cast), totals (pixels, rays, below, shadow_rays, misses), px (pixels()), R (m, samples, 4): the records
    (Gw L, x5), kind (m, samples), below (m, samples), Gw (m, samples)). order: the samples' order in the sums (default 0, 1, ...)"""
    Hh, Ww = g["position"].shape[:2]
    n = params["samples"]
    px = pixels(g, view, meshes, params)
    rows, m = px["rows"], len(px["rows"])
    ss = samples(g, view, px, n)
    R = np.zeros((m, n, 4), np.float32)
    kind = np.full((m, n), DARK, np.uint8)
    below = np.stack([s["below"] for s in ss], axis=1) if m else np.zeros((0, n), bool)
    Gw = np.stack([s["Gw"] for s in ss], axis=1) if m else np.zeros((0, n), np.float32)
    sel = np.nonzero(~below.reshape(-1))[0]  # ray q * n + s
    shadow_rays = 0
    if len(sel):
        q, s = sel // n, sel % n
        d = np.stack([ss[k]["d"] for k in range(n)], axis=1).reshape(-1, 3)[sel]
        L, kd, shadow_rays = radiance(oracle, meshes, g, view, rows[q], px["Nn"][q], d, params["max_radiance"], furnace)
        with np.errstate(all="ignore"):
            R[q, s, :3] = Gw[q, s][:, None] * L
        R[q, s, 3] = np.stack([ss[k]["x5"] for k in range(n)], axis=1).reshape(-1)[sel]
        kind[q, s] = kd
    counts = np.zeros((Hh * Ww, 4), np.uint8)
    S, Bi = np.zeros((Hh * Ww, 3), np.float32), np.zeros((Hh * Ww, 3), np.float32)
    cast = np.zeros(Hh * Ww, bool)
    re = np.full(Hh * Ww, -1, np.int32)
    if m:
        cast[rows] = True
        re[rows] = px["re"]
        for k in range(4):
            counts[rows, k] = (kind == k).sum(axis=1)
        S[rows], Bi[rows] = sums(R, order)
    totals = (m, len(sel), int(below.sum()), int(shadow_rays), int((kind == MISSED).sum()))
    return dict(counts=counts.reshape(Hh, Ww, 4), S=S.reshape(Hh, Ww, 3), Bi=Bi.reshape(Hh, Ww, 3), cast=cast.reshape(Hh, Ww), re=re.reshape(Hh, Ww),
                totals=totals, px=px, R=R, kind=kind, below=below, Gw=Gw)


def sums(R, order=None):
    """S = (sum R_s (1 - x5_s)) / (float)samples and Bi = (sum R_s x5_s) / (float)samples, each from its first term, in sample order"""
    n = R.shape[1]
    order = list(range(n)) if order is None else list(order)
    with np.errstate(all="ignore"):
        term = lambda s: (R[:, s, :3] * (F(1.0) - R[:, s, 3])[:, None], R[:, s, :3] * R[:, s, 3][:, None])
        S, Bi = term(order[0])
        for s in order[1:]:
            a, b = term(s)
            S, Bi = S + a, Bi + b
        return S / F(n), Bi / F(n)


def filter(g, got, params, flag=None):
    """Sf, Bf: UH_HYBRID_GLOSSY_SCALE and _BIAS (H, W, 4) float32, w = 1 where the pixel cast, else (0, 0, 0, 0), from gather()'s dict. A
    pixel of radius re == 0 (or blur_radius 0) keeps S and Bi. Else the mean over the taps (dx, dy) in [-re, re]^2, dy outer: the centre,
    and every tap in the frame that cast, has max(|dx|, |dy|) <= its own re and passes both thresholds against the centre; float32 sums
    from 0 in that order, divided by the tap count. Also returns dict(tainted: some counting tap has flag (H, W) bool, dropped: some tap
    failed the re_tap rule alone)"""
    Hh, Ww = g["position"].shape[:2]
    Nn, _ = ao.normals(g)
    Nn, P = Nn.reshape(Hh, Ww, 3), g["position"][..., :3]
    cast, re, S, Bi = got["cast"], got["re"], got["S"], got["Bi"]
    rmax = int(params["blur_radius"])
    flag = np.zeros((Hh, Ww), bool) if flag is None else flag
    tS, tB, taps = np.zeros((Hh, Ww, 3), np.float32), np.zeros((Hh, Ww, 3), np.float32), np.zeros((Hh, Ww), np.uint32)
    tainted, dropped = np.zeros((Hh, Ww), bool), np.zeros((Hh, Ww), bool)
    with np.errstate(all="ignore"):
        for dy in range(-rmax, rmax + 1):
            for dx in range(-rmax, rmax + 1):
                reach = max(abs(dx), abs(dy))
                mine = cast & (re >= reach)  # the tap lies in this pixel's own window
                if dx == 0 and dy == 0:
                    ok = cast.copy()
                else:
                    Pt, Nt = gi._shifted(P, dx, dy, 0.0), gi._shifted(Nn, dx, dy, 0.0)
                    rest = mine & gi._shifted(cast, dx, dy, False) & (hr.dot(Nt, Nn) >= F(params["blur_normal_cos"])) & (np.abs(hr.dot(Pt - P, Nn)) <= F(params["blur_plane"]))
                    ok = rest & (gi._shifted(re, dx, dy, -1) >= reach)
                    dropped |= rest & ~ok
                tS = np.where(ok[..., None], tS + gi._shifted(S, dx, dy, 0.0), tS)
                tB = np.where(ok[..., None], tB + gi._shifted(Bi, dx, dy, 0.0), tB)
                taps += ok
                tainted |= ok & gi._shifted(flag, dx, dy, False)
        n = taps.astype(np.float32)[..., None]
        keep = (re == 0)[..., None]
        Sf, Bf = np.where(keep, S, tS / n), np.where(keep, Bi, tB / n)
    out_s, out_b = np.zeros((Hh, Ww, 4), np.float32), np.zeros((Hh, Ww, 4), np.float32)
    out_s[..., :3], out_b[..., :3] = np.where(cast[..., None], Sf, F(0.0)), np.where(cast[..., None], Bf, F(0.0))
    out_s[..., 3] = out_b[..., 3] = cast
    return out_s, out_b, dict(tainted=tainted & cast, dropped=dropped & cast)


def composite(g, ssao_img, deferred, Sf, Bf, view, meshes, intensity):
    """deferred_output after the pass, from the output it adds to: for every pixel that cast (Sf.w == 1), F0 = 0.04 (1 - metallic) + base
    metallic, rgb += (((F0 Sf + Bf) intensity) occlusion) [ssao texel / 65535]; alpha untouched. Returns it and the pixels touched"""
    Hh, Ww = g["position"].shape[:2]
    R, A = g["pbr"].reshape(-1, 4), g["albedo"].reshape(-1, 4)
    mf, _, _, bc = material_table(g, meshes)
    out = deferred.copy().reshape(-1, 4)
    S4, B4 = Sf.reshape(-1, 4), Bf.reshape(-1, 4)
    with np.errstate(all="ignore"):
        metallic, occlusion = R[:, 0] * mf, R[:, 2]
        base = fr.gamma_table()[A[:, :3]] * bc
        F0 = np.full((len(R), 3), F(0.04), np.float32) * (F(1.0) - metallic)[:, None] + base * metallic[:, None]
        add = (F0 * S4[:, :3] + B4[:, :3]) * F(intensity)
        add = add * occlusion[:, None]
        if view.ssao_enabled == 1:
            add = add * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
        touched = S4[:, 3] != 0
        out[touched, :3] = out[touched, :3] + add[touched]
    return out.reshape(Hh, Ww, 4), touched.reshape(Hh, Ww)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def _factor_scene_class():
    from rust_renderer_amd.scenes import Scene

    class FactorScene(Scene):
        """every mesh reads a metallic-roughness map whose texel is (g, b) = (1, 1) where the default's is (1, 0): pbr.r * metallic_factor
        and pbr.g * roughness_factor are the mesh's own factors"""

        def upload(self, renderer):
            defaults = renderer.initialize()
            saved = defaults["metallic_roughness"]
            defaults["metallic_roughness"] = renderer.add_texture(np.array([0, 255, 255, 255], np.uint8).reshape(1, 1, 4))
            try:
                return Scene.upload(self, renderer)
            finally:
                defaults["metallic_roughness"] = saved

    return FactorScene


def mirror_floor_scene():
    """rtao_reference's bare floor with roughness_factor 0, metallic 1 and base colour 1: every sample of a pixel is its mirror ray, which misses"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, quad

    fv, fi = quad((-23.0, 0.0, 19.0), (41.0, 0.0, 0.0), (0.0, 0.0, -43.0))
    cam = rr.camera.Camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), 60.0, W / H, 0.01, 1000.0)
    mesh = Mesh(fv, fi, rr.LAMBERTIAN, base_color=(1.0, 1.0, 1.0, 1.0), metallic=1.0, roughness=0.0)
    return _factor_scene_class()("glossy_mirror_floor", [(Model([mesh], []), None)], [], cam)


def inward_box_scene(roughness=0.25):
    """rtao_reference's closed box with a roughness inside the default window: every cast ray meets a wall, every sun ray is occluded.
    (At 0.25 that holds of every ray at 67 x 41 and at WALK_BOX_SIZE, tests/test_glossy_cpu.py; at 0.4 and 0.5 one to three hits in
    200,000 lie within the sun ray's tmin of an edge of the box, and their sun rays start behind the adjacent wall.)"""
    s = ao.inward_box_scene()
    s.models[0][0].meshes[0].roughness = roughness
    s.name = "glossy_inward_box"
    return s


def emissive_box_scene(roughness=0.5):
    """rtgi_reference's box with the emissive wall behind the camera, the other walls at `roughness`"""
    s = gi.emissive_box_scene()
    s.models[0][0].meshes[0].roughness = roughness
    s.name = "glossy_emissive_box"
    return s


GALLERY_SUN = gi.COURTYARD_SUN
GALLERY_MESHES = dict(floor_left=0, floor_right=1, back=2, left=3, right=4, canopy=5, block=6, plinth=7, ball=8, lamp=9)
GALLERY_SIZE = (2 * W, 2 * H)   # 134 x 82: the frame of the gallery's tests, at which every adequacy condition holds at one sample per pixel
GALLERY_BLUR_ROUGHNESS = 0.4  # with it the radii of the gallery's roughnesses 0, 0.15 and 0.4 are 0, 1 and blur_radius (at the default 3)


def gallery_scene():
    """rtgi_reference's courtyard as a gallery of factors, seen from higher up so that the floor mirrors the canopy's opening: a checkered
    floor in two coplanar halves - the left at roughness 0.4, the right polished and metallic (0.15, 1), so the filter's radius changes
    across a seam no threshold sees -, the red back wall and the left wall at 0.4 (the left one seen at a grazing angle: below samples),
    the right wall and the one behind the camera at 0.8, above the default max_roughness, a canopy with an opening of 4 x 3.5, a metallic
    block at 0.15, a mirror-like dielectric plinth (0), a type-1 metal ball, which holds rt_reflections' mirror, and a type-3 lamp panel
    before the back wall"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, box, icosphere, merge, quad

    fl = quad((-3.0, 0.0, 3.0), (3.0, 0.0, 0.0), (0.0, 0.0, -6.0), nu=1, nv=2, uv_scale=(2.0, 4.0))
    fr_ = quad((0.0, 0.0, 3.0), (3.0, 0.0, 0.0), (0.0, 0.0, -6.0), nu=1, nv=2, uv_scale=(2.0, 4.0))
    back = quad((-3.0, 0.0, -3.0), (6.0, 0.0, 0.0), (0.0, 3.0, 0.0))
    left = quad((-3.0, 0.0, -3.0), (0.0, 3.0, 0.0), (0.0, 0.0, 6.0))
    right = merge([quad((3.0, 0.0, -3.0), (0.0, 0.0, 6.0), (0.0, 3.0, 0.0)), quad((-3.0, 0.0, 3.0), (0.0, 3.0, 0.0), (6.0, 0.0, 0.0))])
    canopy = merge([quad((-3.0, 3.0, -3.0), (6.0, 0.0, 0.0), (0.0, 0.0, 1.0)), quad((-3.0, 3.0, 1.5), (6.0, 0.0, 0.0), (0.0, 0.0, 1.5)),
                    quad((-3.0, 3.0, -2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 3.5)), quad((2.0, 3.0, -2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 3.5))])
    sv, si = icosphere(2)
    lamp = quad((-2.8, 0.6, -2.97), (3.2, 0.0, 0.0), (0.0, 1.6, 0.0))
    M = lambda vi, kind, base, rough, metal, **kw: Mesh(*vi, kind, base_color=base, roughness=rough, metallic=metal, **kw)
    meshes = [M(fl, rr.LAMBERTIAN, (1.0, 1.0, 1.0, 1.0), 0.4, 0.0, texture=0), M(fr_, rr.LAMBERTIAN, (1.0, 1.0, 1.0, 1.0), 0.15, 1.0, texture=0),
              M(back, rr.LAMBERTIAN, (0.9, 0.25, 0.2, 1.0), 0.4, 0.0), M(left, rr.LAMBERTIAN, (0.8, 0.8, 0.75, 1.0), 0.4, 0.0),
              M(right, rr.LAMBERTIAN, (0.8, 0.8, 0.75, 1.0), 0.8, 0.0), M(canopy, rr.LAMBERTIAN, (0.6, 0.6, 0.6, 1.0), 0.8, 0.0),
              M(box((-1.0, 0.5, -2.2), (0.5, 0.5, 0.5)), rr.LAMBERTIAN, (0.3, 0.7, 0.4, 1.0), 0.15, 1.0),
              M(box((1.1, 0.2, 0.2), (0.8, 0.2, 0.6)), rr.LAMBERTIAN, (0.8, 0.8, 0.3, 1.0), 0.0, 0.0),
              M((sv, si), rr.METAL, (0.9, 0.9, 0.9, 1.0), 0.15, 1.0, transform=rr.transform3x4((0.7, 0.7, 0.7), (-1.4, 0.7, 0.3))),
              M(lamp, rr.DIFFUSE_LIGHT, (1.0, 1.0, 1.0, 1.0), 1.0, 0.0)]
    cam = rr.camera.Camera((0.6, 2.6, 2.7), (-0.3, 0.0, -0.5), 70.0, W / H, 0.01, 1000.0)
    return _factor_scene_class()("glossy_gallery", [(Model(meshes, [gi.checker()]), None)], [], cam)


# frames at which the persistent walks refill (tests/test_gpu_glossy_chunks.py), as rtgi_reference has them
WALK_LANES = gi.WALK_LANES
WALK_BOX_SIZE = gi.WALK_BOX_SIZE
WALK_EMISSIVE_SIZE = gi.WALK_EMISSIVE_SIZE
WALK_GALLERY_SIZE = (163, 101)  # the gallery at 16 samples: more than one grid of sun rays, so k_rtgi_shadow refills on this pass's buffers


def scene_view(scene, width=W, height=H, **kw):
    """rtgi_reference.scene_view; the gallery has the courtyard's sun"""
    v = gi.scene_view(scene, width, height, **kw)
    if scene.name == "glossy_gallery":
        s = np.array(GALLERY_SUN, np.float64)
        v.sun_dir[:] = [float(x) for x in np.float32(s / np.linalg.norm(s))]
    return v

"""CPU restatement of one-bounce ray-traced diffuse GI (uh_render_hybrid's UH_HYBRID_RTGI): which pixels cast, their cosine-weighted
hemisphere rays, the radiance of each ray (sky, emitter, sun-lit or dark hit), the ray counts, the per-pixel mean in sample order, the
filter and the composite into deferred_output, in numpy float32 in the order DESIGN.md section 2 "Ray-traced diffuse GI" pins.
Composed from tests/rtao_reference.py (normals, _sphere_points with the XORed frame word), tests/hybrid_reference.py (trace, offset_ray,
_uv, sample, the world-normal arithmetic), tests/hybrid_frame_reference.py (light_records, gamma_table) and the oracle's sky and
frame_number. Each function takes the G-buffer as an argument, so a test can feed it the device's own. With the scenes the tests use.
Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao

F = np.float32
SEED_XOR = 0x52544749
SUNLIT, DARK, EMITTER, MISSED = 0, 1, 2, 3  # the bytes of a pixel's counts, in order
W, H = ao.W, ao.H  # 67 x 41: neither a multiple of the 32 x 8 filter tile nor of 64


def default_params(**kw):
    """uh_rtgi_default_params, with `kw` over it"""
    p = dict(samples=2, blur_radius=3, max_radiance=16.0, intensity=1.0, blur_normal_cos=0.9, blur_plane=0.05)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def directions(g, view, samples):
    """the pixels that cast (indices into the flattened frame), their Nn (m, 3), and the ray directions (m, samples, 3):
    d = normalize(Nn + normalize(u)), u = randomPointInUnitSphere of initRNG(px, py, W, (frame * 64 + s) ^ SEED_XOR); Nn itself where
    |Nn + normalize(u)|^2 is not >= 1e-12"""
    Hh, Ww = g["position"].shape[:2]
    Nn, cast = ao.normals(g)
    rows = np.nonzero(cast)[0]
    frame = oa.frame_number(view)
    nn = Nn[rows]
    d = np.empty((len(rows), samples, 3), np.float32)
    with np.errstate(all="ignore"):
        for s in range(samples):
            word = ((frame * 64 + s) ^ SEED_XOR) & 0xFFFFFFFF  # _sphere_points seeds with frame' * 64 + s'
            u = hr.normalize(ao._sphere_points(Ww, Hh, word >> 6, word & 63)[rows])
            w = nn + u
            d[:, s] = np.where((hr.dot(w, w) >= F(1e-12))[:, None], hr.normalize(w), nn)
    return rows, nn, d


def clamp(L, max_radiance):
    """L > 0 ? L : 0 (a NaN, a negative and -0 become +0), then the cap"""
    with np.errstate(all="ignore"):
        return np.minimum(np.where(L > 0, L, F(0.0)), F(max_radiance)).astype(np.float32)


def rays(oracle, meshes, g, view, samples, max_radiance, furnace=False):
    """every ray of the pass: dict(rows (m,), L (m, samples, 3) float32 as stored, kind (m, samples) of SUNLIT / DARK / EMITTER / MISSED,
    shadowed (m, samples): dark because its sun ray was occluded, shadow_rays: the sun rays cast, mesh (m, samples): the mesh the ray met
    (hybrid_reference.MISS where none), and of the hits that are shaded (no emitter, no furnace) Nh (m, samples, 3), the world normal
    after its turn toward the ray (NaN elsewhere), and flipped (m, samples): the turn took place, dot(Nh before it, d) > 0)"""
    rows, nn, d = directions(g, view, samples)
    m = len(rows)
    L = np.zeros((m * samples, 3), np.float32)
    kind = np.full(m * samples, DARK, np.uint8)
    shadowed = np.zeros(m * samples, bool)
    hit_mesh = np.full(m * samples, hr.MISS, np.uint32)
    hit_Nh = np.full((m * samples, 3), np.nan, np.float32)
    flipped = np.zeros(m * samples, bool)
    out = dict(rows=rows, L=L.reshape(m, samples, 3), kind=kind.reshape(m, samples), shadowed=shadowed.reshape(m, samples), shadow_rays=0,
               mesh=hit_mesh.reshape(m, samples), Nh=hit_Nh.reshape(m, samples, 3), flipped=flipped.reshape(m, samples))
    if not m:
        return out
    o = np.repeat(hr.offset_ray(g["position"][..., :3].reshape(-1, 3)[rows], nn), samples, axis=0)
    d = d.reshape(-1, 3)
    t, u, v, mesh, prim = hr.trace(oracle, o, d)
    miss = mesh == hr.MISS
    hit_mesh[:] = mesh
    kind[miss] = MISSED
    for k in np.nonzero(miss)[0]:
        L[k] = 1.0 if furnace else oa.sky(o[k], d[k], view.sun_dir[:])  # IntegrateScattering(o, d, 999999999, sun), unclamped
    hit = np.nonzero(~miss)[0]
    types = np.array([meshes[int(i)]["type"] for i in mesh[hit]], np.float32)
    emit = hit[types == 3.0]
    kind[emit] = EMITTER
    L[emit] = 1.0  # reference.rchit:85-89: color = vec3(1.0), the path ends
    rest = hit[types != 3.0]
    if len(rest) and not furnace:
        with np.errstate(all="ignore"):
            b0, b1, b2 = (F(1.0) - u[rest]) - v[rest], u[rest], v[rest]
            hm, hp = mesh[rest], prim[rest]
            uu, vv = hr._uv(meshes, hm, hp, b0, b1, b2)
            tex = hr.sample(oracle, np.array([meshes[int(i)]["diffuse_map"] for i in hm], np.uint32), uu, vv)
            albedo = tex * np.array([meshes[int(i)]["base_color"] for i in hm], np.float32).reshape(-1, 3)  # rchit:41-42
            Nh = np.zeros((len(rest), 3), np.float32)
            for i in np.unique(hm):  # rchit:31-37
                sel = hm == i
                M = meshes[int(i)]
                tri = M["indices"].reshape(-1, 3)[hp[sel]]
                vn = [M["vertices"]["normal"][tri[:, k], :3].astype(np.float32) for k in range(3)]
                n = (vn[0] * b0[sel][:, None] + vn[1] * b1[sel][:, None]) + vn[2] * b2[sel][:, None]
                Nh[sel] = hr.normalize(hr.inverse_transpose_mul(hr.invert3x3(M["world"]), n))
            flipped[rest] = hr.dot(Nh, d[rest]) > 0
            Nh = np.where(flipped[rest][:, None], -Nh, Nh)
            hit_Nh[rest] = Nh
            X = o[rest] + t[rest][:, None] * d[rest]
            sun = hr.sun_direction(view)
            ndl = hr.dot(Nh, np.broadcast_to(sun, Nh.shape))
            NdotL = np.where(ndl > 0, ndl, F(0.0))  # max(dot, 0); a NaN is 0
            cand = NdotL > 0
            ci = np.nonzero(cand)[0]
            _, _, _, blocker, _ = hr.trace(oracle, hr.offset_ray(X[ci], Nh[ci]), np.broadcast_to(sun, (len(ci), 3)))
            occluded = blocker != hr.MISS
            sun_rec = fr.light_records(view, [])[0]
            rad_sun = sun_rec["color"] * F(1.0)  # pbr_lighting.glsl:59: color * attenuation, 1 for a directional light
            lit = ci[~occluded]
            L[rest[lit]] = ((albedo[lit] / fr.PI) * rad_sun[None, :]) * NdotL[lit][:, None]
            kind[rest[lit]] = SUNLIT
            shadowed[rest[ci[occluded]]] = True
            out["shadow_rays"] = len(ci)
    L[:] = clamp(L, max_radiance)
    return out


def mean(L):
    """E = (L_0 + L_1 + ... + L_{samples-1}) / (float)samples, in sample order: (m, 3)"""
    acc = L[:, 0].copy()
    for s in range(1, L.shape[1]):
        acc = acc + L[:, s]
    return acc / F(L.shape[1])


def gather(oracle, meshes, g, view, params, furnace=False):
    """the pass up to its filter: counts (H, W, 4) uint8, E (H, W, 3) float32 (0 where nothing was cast), cast (H, W), totals (pixels, rays,
    shadow_rays, misses) and the rays' record (rays())"""
    Hh, Ww = g["position"].shape[:2]
    r = rays(oracle, meshes, g, view, params["samples"], params["max_radiance"], furnace)
    counts = np.zeros((Hh * Ww, 4), np.uint8)
    E = np.zeros((Hh * Ww, 3), np.float32)
    cast = np.zeros(Hh * Ww, bool)
    rows = r["rows"]
    if len(rows):
        cast[rows] = True
        for k in range(4):
            counts[rows, k] = (r["kind"] == k).sum(axis=1)
        E[rows] = mean(r["L"])
    totals = (len(rows), len(rows) * params["samples"], r["shadow_rays"], int((r["kind"] == MISSED).sum()))
    return counts.reshape(Hh, Ww, 4), E.reshape(Hh, Ww, 3), cast.reshape(Hh, Ww), totals, r


def _shifted(a, dx, dy, fill):
    """a[y + dy, x + dx] where that lies in the frame, else fill"""
    Hh, Ww = a.shape[:2]
    out = np.full_like(a, fill)
    if abs(dx) >= Ww or abs(dy) >= Hh:
        return out
    ys, yd = (slice(max(dy, 0), Hh + min(dy, 0)), slice(max(-dy, 0), Hh + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), Ww + min(dx, 0)), slice(max(-dx, 0), Ww + min(-dx, 0)))
    out[yd, xd] = a[ys, xs]
    return out


def filter(g, E, params, flag=None):
    """Ef: UH_HYBRID_GI_RADIANCE (H, W, 4) float32, w = 1 where the pixel cast, else (0, 0, 0, 0). blur_radius 0: E. r > 0: the mean of E
    over the taps (dx, dy) in [-r, r]^2, dy outer, that lie in the frame, cast themselves and pass both thresholds against the centre;
    the centre always counts; float32 sum in that order, divided by the tap count. flag (H, W) bool: also returns, per pixel, whether
    any tap that counted has it"""
    Hh, Ww = g["position"].shape[:2]
    Nn, cast = ao.normals(g)
    cast, Nn, P = cast.reshape(Hh, Ww), Nn.reshape(Hh, Ww, 3), g["position"][..., :3]
    r = int(params["blur_radius"])
    out = np.zeros((Hh, Ww, 4), np.float32)
    total, taps = np.zeros((Hh, Ww, 3), np.float32), np.zeros((Hh, Ww), np.uint32)
    any_flag = np.zeros((Hh, Ww), bool)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    ok = np.ones((Hh, Ww), bool)
                else:
                    Pt, Nt = _shifted(P, dx, dy, 0.0), _shifted(Nn, dx, dy, 0.0)
                    ok = _shifted(cast, dx, dy, False) & (hr.dot(Nt, Nn) >= F(params["blur_normal_cos"])) & (np.abs(hr.dot(Pt - P, Nn)) <= F(params["blur_plane"]))
                total = np.where(ok[..., None], total + _shifted(E, dx, dy, 0.0), total)
                taps += ok
                if flag is not None:
                    any_flag |= ok & _shifted(flag, dx, dy, False)
        mean_ = total / taps.astype(np.float32)[..., None]
    out[..., :3] = np.where(cast[..., None], mean_, F(0.0))
    out[..., 3] = cast
    return (out, any_flag & cast) if flag is not None else out


def composite(g, ssao_img, deferred, Ef, view, meshes, intensity):
    """deferred_output after the pass, from the deferred pass's own output: for every pixel that cast (Ef.w == 1) and is no metal pixel
    under raytracing_supported == 1, rgb += (((base (1 - metallic)) Ef) intensity) occlusion [ssao texel / 65535]; alpha untouched"""
    Hh, Ww = g["position"].shape[:2]
    R, A = g["pbr"].reshape(-1, 4), g["albedo"].reshape(-1, 4)
    material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    table = lambda key, default: np.where(valid, np.array([m[key] for m in meshes] or [default], np.float32)[idx], F(default))
    mf, typ = table("metallic", 1.0), table("type", 0.0)
    bc = np.where(valid[:, None], np.array([m["base_color"] for m in meshes] or [np.ones(3)], np.float32)[idx], F(1.0))
    out = deferred.copy().reshape(-1, 4)
    E4 = Ef.reshape(-1, 4)
    with np.errstate(all="ignore"):
        metallic, occlusion = R[:, 0] * mf, R[:, 2]
        base = fr.gamma_table()[A[:, :3]] * bc
        add = ((base * (F(1.0) - metallic)[:, None]) * E4[:, :3]) * F(intensity)
        add = add * occlusion[:, None]
        if view.ssao_enabled == 1:
            add = add * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
        touched = (E4[:, 3] != 0) & ~((view.raytracing_supported == 1) & (typ == 1.0))
        out[touched, :3] = out[touched, :3] + add[touched]
    return out.reshape(Hh, Ww, 4), touched.reshape(Hh, Ww)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
floor_scene = ao.floor_scene            # every ray misses
inward_box_scene = ao.inward_box_scene  # every ray hits, and every sun ray is occluded
EMISSION = 1.0                          # what a ray that meets a material of type 3 brings, per channel


def _inward_walls(skip=None, only=None):
    """the six walls of rtao_reference's box as scenes.box lays them out, normals inward; `skip` / `only`: (axis, sign) of one wall"""
    from rust_renderer_amd.scenes import merge, quad

    c, h = np.asarray(ao.BOX_CENTRE, np.float64), np.asarray(ao.BOX_HALF, np.float64)
    parts = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            if (axis, sign) == skip or (only is not None and (axis, sign) != only):
                continue
            a, b = (axis + 1) % 3, (axis + 2) % 3
            eu, ev = np.zeros(3), np.zeros(3)
            eu[a], ev[b] = 2 * h[a], 2 * h[b]
            o = c.copy()
            o[axis] += sign * h[axis]
            o[a] -= h[a]
            o[b] -= h[b]
            parts.append(quad(o, eu, ev, 1, 1, flip=sign < 0))
    v, i = merge(parts)
    v["normal"][:, :3] *= -1.0
    return v, i


def emissive_box_scene():
    """the inward box with the wall behind the camera (z = +1.2) of material type 3: the wall the camera looks at faces it"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene

    wv, wi = _inward_walls(skip=(2, 1.0))
    ev, ei = _inward_walls(only=(2, 1.0))
    cam = rr.camera.Camera((0.1, 1.05, 0.6), (0.0, 1.0, -1.2), 30.0, W / H, 0.01, 1000.0)
    meshes = [Mesh(wv, wi, rr.LAMBERTIAN, base_color=(0.7, 0.7, 0.8, 1.0)), Mesh(ev, ei, rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0))]
    return Scene("rtgi_emissive_box", [(Model(meshes, []), None)], [], cam)


COURTYARD_SUN = (0.25, 0.6, 0.75)  # toward the sun: its light comes down through the opening onto the back wall and the floor before it


def checker(size=8, a=(230, 220, 200, 255), b=(60, 90, 140, 255)):
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    return np.ascontiguousarray(np.where(((x + y) % 2 == 0)[..., None], np.array(a, np.uint8), np.array(b, np.uint8)))


def courtyard_scene():
    """a walled yard, 6 x 6 and 3 high, seen from inside: a checkered floor (its map repeats four times each way, so uv matters), a red back
    wall, three pale walls, a canopy over all of it but an opening of 3 x 2.5 through which the sun, at an angle, lights the foot of the
    back wall and a strip of the floor before it, and the sky shows; a block stands in the light and shadows part of the floor"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box, merge, quad

    floor = quad((-3.0, 0.0, 3.0), (6.0, 0.0, 0.0), (0.0, 0.0, -6.0), nu=2, nv=2, uv_scale=(4.0, 4.0))
    back = quad((-3.0, 0.0, -3.0), (6.0, 0.0, 0.0), (0.0, 3.0, 0.0))
    sides = merge([quad((-3.0, 0.0, -3.0), (0.0, 3.0, 0.0), (0.0, 0.0, 6.0)), quad((3.0, 0.0, -3.0), (0.0, 0.0, 6.0), (0.0, 3.0, 0.0)),
                   quad((-3.0, 0.0, 3.0), (0.0, 3.0, 0.0), (6.0, 0.0, 0.0))])
    canopy = merge([quad((-3.0, 3.0, -3.0), (6.0, 0.0, 0.0), (0.0, 0.0, 2.0)), quad((-3.0, 3.0, 1.5), (6.0, 0.0, 0.0), (0.0, 0.0, 1.5)),
                    quad((-3.0, 3.0, -1.0), (1.5, 0.0, 0.0), (0.0, 0.0, 2.5)), quad((1.5, 3.0, -1.0), (1.5, 0.0, 0.0), (0.0, 0.0, 2.5))])
    block = box((-1.0, 0.5, -2.2), (0.5, 0.5, 0.5))
    meshes = [Mesh(*floor, rr.LAMBERTIAN, base_color=(1.0, 1.0, 1.0, 1.0), texture=0), Mesh(*back, rr.LAMBERTIAN, base_color=(0.9, 0.25, 0.2, 1.0)),
              Mesh(*sides, rr.LAMBERTIAN, base_color=(0.8, 0.8, 0.75, 1.0)), Mesh(*canopy, rr.LAMBERTIAN, base_color=(0.6, 0.6, 0.6, 1.0)),
              Mesh(*block, rr.LAMBERTIAN, base_color=(0.3, 0.7, 0.4, 1.0))]
    cam = rr.camera.Camera((0.6, 1.7, 2.7), (-0.6, 0.7, -2.0), 70.0, W / H, 0.01, 1000.0)
    return Scene("rtgi_courtyard", [(Model(meshes, [checker()]), None)], [], cam)


# ---- the turned scene: back faces, a mirrored instance, the odd materials, zero normals, the clamp -----------------------------------
TURNED_SUN = (-0.35, 0.7, 0.6)  # toward the sun: from the camera's side, so the wall below is lit on the side its vertex normals face away from
TURNED_MESHES = dict(floor=0, wall=1, mirrored=2, metal=3, dielectric=4, pbr=5, zero=6, clamp=7)
CLAMP_COLOR = (-1.0, 3.0e38, float("nan"), 1.0)  # a sunlit ray brings (negative, beyond every finite cap, NaN): stored as (+0, max_radiance, +0)


def turned_scene():
    """what no other scene of the pass has, one mesh each. A floor; a free-standing wall of one sheet whose vertex normals point away from
    the camera and the floor before it (-z), so every floor ray meets its back, and the sun (TURNED_SUN) stands on the camera's side: the
    hit is sunlit only if its normal is turned toward the ray. Its checker map is addressed with uv in [-1.2, 1.8]. A box under a
    mirrored, rotated and non-uniformly scaled instance (negative determinant). A metal sphere, a dielectric box and a box of material
    type 4 on the floor: hits on them are shaded as any other hit. A sheet over the camera's head, outside its view, whose vertex
    normals are all zero: Nh is NaN, the hit is dark and casts no sun ray. And a panel beside the floor, outside the view, that faces the
    sun with the base colour CLAMP_COLOR: its sunlit hits run into every branch of the clamp."""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box, icosphere, quad

    floor = quad((-5.0, 0.0, 5.0), (10.0, 0.0, 0.0), (0.0, 0.0, -10.0), nu=2, nv=2)
    wv, wi = quad((2.0, 0.0, -1.5), (-4.0, 0.0, 0.0), (0.0, 2.0, 0.0), nu=2, nv=2)
    assert (wv["normal"][:, 2] == -1.0).all()
    wv["uv"][:] = wv["uv"] * np.float32(3.0) - np.float32(1.2)
    rot = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]], np.float32)
    mirrored = rr.transform3x4((-1.3, 0.8, 0.6), (-2.4, 0.4, 0.6), rot)
    sv, si = icosphere(1)
    zv, zi = quad((-2.0, 3.5, 5.0), (4.0, 0.0, 0.0), (0.0, 0.0, -3.0), nu=2, nv=2)
    zv["normal"][:] = 0.0
    cv, ci = quad((4.5, 0.0, 2.5), (0.0, 0.0, 1.9), (0.0, 2.5, 0.0))
    assert (cv["normal"][:, 0] == -1.0).all()
    meshes = [Mesh(*floor, rr.LAMBERTIAN, base_color=(0.8, 0.8, 0.8, 1.0)),
              Mesh(wv, wi, rr.LAMBERTIAN, base_color=(1.0, 0.9, 0.8, 1.0), texture=0),
              Mesh(*box((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)), rr.LAMBERTIAN, base_color=(0.3, 0.7, 0.4, 1.0), transform=mirrored),
              Mesh(sv, si, rr.METAL, 0.1, base_color=(0.9, 0.6, 0.3, 1.0), transform=rr.transform3x4((0.5, 0.5, 0.5), (2.3, 0.5, 0.8))),
              Mesh(*box((1.1, 0.35, 1.9), (0.35, 0.35, 0.35)), rr.DIELECTRIC, 1.5, base_color=(0.9, 0.9, 1.0, 1.0)),
              Mesh(*box((-1.2, 0.3, 1.9), (0.3, 0.3, 0.3)), rr.PBR, base_color=(0.6, 0.5, 0.9, 1.0), metallic=0.5, roughness=0.4),
              Mesh(zv, zi, rr.LAMBERTIAN, base_color=(0.5, 0.5, 0.5, 1.0)),
              Mesh(cv, ci, rr.LAMBERTIAN, base_color=CLAMP_COLOR)]
    cam = rr.camera.Camera((0.0, 2.2, 4.5), (0.0, 0.3, 0.0), 60.0, W / H, 0.01, 1000.0)
    return Scene("rtgi_turned", [(Model(meshes, [checker()]), None)], [], cam)


SUNS = {"rtgi_courtyard": COURTYARD_SUN, "rtgi_turned": TURNED_SUN}

# ---- frames at which the persistent walks refill (tests/test_gpu_walk_chunks.py; their adequacy: tests/test_rtgi_cpu.py) ------------------
WALK_LANES = 65536               # the lanes of a persistent grid at option "trace_blocks_per_cu" = 1 on 256 CUs
WALK_BOX_SIZE = (131, 97)        # the closed box at 16 samples: 203,312 rays, 3.1 grids
WALK_EMISSIVE_SIZE = (263, 167)  # the emissive box at 3 samples: 131,763 rays, 2.01 grids, a last chunk of 51
WALK_YARD_SIZE = (183, 113)      # the courtyard at 16 samples: the smallest odd width at 67 : 41 with two grids of sun rays
WALK_AO_SIZE = (71, 45)          # the closed box at RTAO's 64 samples: 204,480 rays, 3.1 grids


def scene_view(scene, width=W, height=H, **kw):
    """hybrid_util.frame_view, with the scene's own sun where it has one (SUNS)"""
    v = scene.make_view(width, height, **kw)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    if scene.name in SUNS:
        s = np.array(SUNS[scene.name], np.float64)
        v.sun_dir[:] = [float(x) for x in np.float32(s / np.linalg.norm(s))]
    return v

"""CPU restatement of the hybrid frame's area lights (uh_render_hybrid's UH_HYBRID_AREA_LIGHTS): the emitter table from the meshes as
uploaded and their transforms, which pixels cast, the picks, points, geometry terms and the two shading halves of their samples, the
shadow verdicts through the oracle, the counts, the per-pixel means in sample order, the filter and the composite into deferred_output,
in numpy float32 in the order DESIGN.md section 2 "Area lights" pins. Composed from tests/hybrid_reference.py (dot, cross, normalize,
offset_ray, the oracle's trace), tests/hybrid_frame_reference.py (the gamma table, PI), tests/rtao_reference.py (normals) and
tests/rtgi_reference.py (the shifted taps). Each function takes the G-buffer as an argument, so a test can feed it the device's own.
With the scenes the tests use. Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao
import rtgi_reference as gi
import rust_renderer_amd as rr

F = np.float32
SEED_XOR = 0x41524541
LIT, OCCLUDED, AWAY = 0, 1, 2  # the bytes of a pixel's counts, in order
PRIM_BITS = 22
W, H = ao.W, ao.H  # 67 x 41: neither a multiple of the 32 x 8 filter tile nor of 64
FLT_MAX = float(np.finfo(np.float32).max)


def default_params(**kw):
    """uh_area_light_default_params, with `kw` over it"""
    p = dict(samples=2, blur_radius=3, show_emitters=1, max_weight=64.0, max_radiance=16.0, intensity=1.0, blur_normal_cos=0.9, blur_plane=0.05)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- the random numbers, vectorised (random.glsl) ----------------------------------------------------------------------------------------
def _u32(x):
    return np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def jenkins_hash(x):
    x = _u32(x)
    x = _u32(x + (x << np.uint64(10)))
    x = x ^ (x >> np.uint64(6))
    x = _u32(x + (x << np.uint64(3)))
    x = x ^ (x >> np.uint64(11))
    return _u32(x + (x << np.uint64(15)))


def init_rng(px, py, width, frame):
    """initRNG(px, py, W, frame) for arrays of pixels: (n,) uint64 holding 32-bit states"""
    d = np.asarray(px).astype(np.float32) * F(1.0) + np.asarray(py).astype(np.float32) * F(width)
    return jenkins_hash(d.astype(np.uint64) ^ jenkins_hash(np.uint64(frame & 0xFFFFFFFF)))


def step(state):
    """one step of the state: (the new state, its 32-bit output word - what randomFloat converts)"""
    s = _u32(state * np.uint64(747796405) + np.uint64(1))
    word = _u32(((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737))
    return s, (word >> np.uint64(22)) ^ word


def to_float(word):
    return word.astype(np.uint32).astype(np.float32) * F(2.3283064365386963e-10)


# ---- the emitter table -------------------------------------------------------------------------------------------------------------------
def world_corners(M):
    """the three corners of every triangle of mesh record M as the tree's packets hold them: (t, 3, 3) float32"""
    tri = M["indices"].reshape(-1, 3)
    pos = M["vertices"]["pos"][:, :3].astype(np.float32)
    c = pos[tri]  # (t, 3 corners, 3)
    w = np.asarray(M["world"], np.float32)
    if np.array_equal(w, rr.identity3x4()):
        return c
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([((w[4 * r] * x + w[4 * r + 1] * y) + w[4 * r + 2] * z) + w[4 * r + 3] for r in range(3)], axis=-1).astype(np.float32)


def table(meshes):
    """dict(keys (N,) uint32, v0, e1, e2 (N, 3) float32, areas (N,) float32, weights, cum (N,) uint32, total, amax, b, x): the emitters in
    slot order - meshes in upload order, primitives in index order"""
    keys, v0, e1, e2 = [], [], [], []
    for mi, M in enumerate(meshes):
        if M["type"] != 3.0:
            continue
        c = world_corners(M)
        keys.append((np.uint32(mi) << np.uint32(PRIM_BITS)) | np.arange(len(c), dtype=np.uint32))
        v0.append(c[:, 0]), e1.append(c[:, 1] - c[:, 0]), e2.append(c[:, 2] - c[:, 0])
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    t = dict(keys=cat(keys, 0, np.uint32), v0=cat(v0, (0, 3), np.float32), e1=cat(e1, (0, 3), np.float32), e2=cat(e2, (0, 3), np.float32))
    n = len(t["keys"])
    with np.errstate(all="ignore"):
        Ng = hr.cross(t["e1"], t["e2"])
        area = F(0.5) * np.sqrt(hr.dot(Ng, Ng))
        area = np.where(area < F(np.inf), area, F(0.0)).astype(np.float32)
    amax = F(area.max()) if n else F(0.0)
    _, x = np.frexp(amax)
    b = 31 - int(max(n, 1) - 1).bit_length()
    q = np.zeros(n, np.uint32)
    pos = area > 0
    scaled = np.trunc(np.ldexp(area[pos], np.int32(b - int(x)))).astype(np.float32)
    q[pos] = np.maximum(scaled.astype(np.uint64), 1).astype(np.uint32)
    cum = np.cumsum(q.astype(np.uint64)).astype(np.uint64)
    total = int(cum[-1]) if n else 0
    assert total <= 1 << 31
    t.update(areas=area, weights=q, cum=cum.astype(np.uint32), total=total, amax=amax, b=b, x=int(x), Ng=Ng.astype(np.float32))
    return t


# ---- which pixels cast, and their samples ------------------------------------------------------------------------------------------------
def materials(g, meshes):
    """per pixel of the flattened frame: metallic factor, roughness factor, type and base colour of the material record uint(pbr.a)"""
    R = g["pbr"].reshape(-1, 4)
    material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    col = lambda key, default: np.where(valid, np.array([m[key] for m in meshes] or [default], np.float32)[idx], F(default))
    bc = np.where(valid[:, None], np.array([m["base_color"] for m in meshes] or [np.ones(3)], np.float32)[idx], F(1.0))
    return col("metallic", 1.0), col("roughness", 1.0), col("type", 0.0), bc.astype(np.float32)


def classify(g, view, meshes, tab):
    """cast (n,) bool: the pixels that cast; emitter (n,) bool: the emitters' own pixels"""
    Nn, geo = ao.normals(g)
    _, _, typ, _ = materials(g, meshes)
    lit = g["position"].reshape(-1, 4)[:, 3] != 0
    emitter = lit & (typ == 3.0)
    cast = geo & ~emitter & ~((view.raytracing_supported == 1) & (typ == 1.0)) & (tab["total"] != 0)
    return cast, emitter


def surface(g, view, meshes, rows):
    """the deferred pass's terms of the pixels `rows`: P, N, V, base and surface_terms' fields"""
    P = g["position"][..., :3].reshape(-1, 3)[rows]
    N = g["normal"][..., :3].reshape(-1, 3)[rows]
    R, A = g["pbr"].reshape(-1, 4)[rows], g["albedo"].reshape(-1, 4)[rows]
    mf, rf, _, bc = (a[rows] for a in materials(g, meshes))
    with np.errstate(all="ignore"):
        metallic, roughness = R[:, 0] * mf, R[:, 1] * rf
        base = fr.gamma_table()[A[:, :3]] * bc
        V = hr.normalize(np.array(view.eye_pos[:], np.float32)[None, :] - P)
        om = F(1.0) - metallic
        F0 = np.full((len(rows), 3), F(0.04), np.float32) * om[:, None] + base * metallic[:, None]
        NdotV = np.maximum(hr.dot(N, V), F(0.0))
        a = roughness * roughness
        a2 = a * a
        r1 = roughness + F(1.0)
        k = (r1 * r1) / F(8.0)
        omk = F(1.0) - k
        return dict(P=P, N=N, V=V, base=base, om=om, F0=F0, a2=a2, a2m1=a2 - F(1.0), k=k, omk=omk, ggxV=NdotV / (NdotV * omk + k), nv4=F(4.0) * NdotV)


def halves(t, l, NdotL, G):
    """d_s and s_s of one light of direction l and radiance (G, G, G) on the surface terms t: ((n, 3), (n, 3))"""
    with np.errstate(all="ignore"):
        N, V = t["N"], t["V"]
        Hv = hr.normalize(V + l)
        NdotH = np.maximum(hr.dot(N, Hv), F(0.0))
        dn = (NdotH * NdotH) * t["a2m1"] + F(1.0)
        dn = (fr.PI * dn) * dn
        NDF = t["a2"] / dn
        Gs = (NdotL / (NdotL * t["omk"] + t["k"])) * t["ggxV"]
        x = np.minimum(np.maximum(F(1.0) - np.maximum(hr.dot(Hv, V), F(0.0)), F(0.0)), F(1.0))
        p5 = ((x * x) * (x * x)) * x
        Fr = t["F0"] + (F(1.0) - t["F0"]) * p5[:, None]
        kD = (F(1.0) - Fr) * t["om"][:, None]
        NG = NDF * Gs
        den2 = t["nv4"] * NdotL + F(0.0001)
        spec = (NG[:, None] * Fr) / den2[:, None]
        rad = np.repeat(G[:, None], 3, axis=1) * NdotL[:, None]
        return (kD * rad).astype(np.float32), (spec * rad).astype(np.float32)


def samples(g, view, meshes, params, tab, dtype=np.float32):
    """every sample of the pass before its shadow ray: dict(rows (m,), pick (m, s), Y (m, s, 3), g0, G, NdotL (m, s), away (m, s) bool, d, s
    (m, s, 3): the two halves, zero where away). dtype float64: the geometry lines (w .. g0) in float64 from the same picks and points"""
    Hh, Ww = g["position"].shape[:2]
    cast, _ = classify(g, view, meshes, tab)
    rows = np.nonzero(cast)[0]
    m, ns = len(rows), int(params["samples"])
    out = dict(rows=rows, pick=np.zeros((m, ns), np.int64), Y=np.zeros((m, ns, 3), np.float32), g0=np.zeros((m, ns), dtype), G=np.zeros((m, ns), dtype),
               NdotL=np.zeros((m, ns), dtype), away=np.ones((m, ns), bool), d=np.zeros((m, ns, 3), np.float32), s=np.zeros((m, ns, 3), np.float32))
    if not m:
        return out
    t = surface(g, view, meshes, rows)
    frame = oa.frame_number(view)
    total = tab["total"]
    T = dtype
    for s in range(ns):
        state = init_rng(rows % Ww, rows // Ww, Ww, (frame * 64 + s) ^ SEED_XOR)
        state, r = step(state)
        state, w1 = step(state)
        state, w2 = step(state)
        u1, u2 = to_float(w1), to_float(w2)
        target = (r * np.uint64(total)) >> np.uint64(32)
        i = np.searchsorted(tab["cum"].astype(np.uint64), target, side="right")
        with np.errstate(all="ignore"):
            fold = u1 + u2 > F(1.0)
            u1, u2 = np.where(fold, F(1.0) - u1, u1), np.where(fold, F(1.0) - u2, u2)
            v0, e1, e2 = tab["v0"][i], tab["e1"][i], tab["e2"][i]
            Y = ((v0 + u1[:, None] * e1) + u2[:, None] * e2).astype(np.float32)
            Ng = hr.cross(e1.astype(T), e2.astype(T))
            ng2 = hr.dot(Ng, Ng)
            w = Y.astype(T) - t["P"].astype(T)
            d2 = hr.dot(w, w)
            dist = np.sqrt(d2)
            l = w / dist[:, None]
            cosL = np.abs(hr.dot(Ng, l)) / np.sqrt(ng2)
            NdotL = hr.dot(t["N"].astype(T), l)
            invpdf = (tab["areas"][i].astype(T) * T(total)) / tab["weights"][i].astype(T)
            g0 = (cosL / d2) * invpdf
            away = ~(d2 > 0) | ~(NdotL > 0) | ~(cosL > 0) | np.isnan(g0)
            G = np.minimum(g0, T(params["max_weight"]))
            out["pick"][:, s], out["Y"][:, s], out["g0"][:, s], out["G"][:, s], out["NdotL"][:, s], out["away"][:, s] = i, Y, g0, G, NdotL, away
            if dtype is np.float32:
                ds, ss = halves(t, l, NdotL, G)
                out["d"][:, s] = np.where(away[:, None], F(0.0), ds)
                out["s"][:, s] = np.where(away[:, None], F(0.0), ss)
    return out


def verdicts(oracle, g, smp):
    """occluded (m, s) bool of the samples that are not away: one any-hit ray from offsetRay(P, Nn) toward Y, tmin 0.001, tmax 0.999 |Y - o|,
    through the oracle's trace (some triangle in the interval: the closest hit decides)"""
    rows, away = smp["rows"], smp["away"]
    occ = np.zeros(away.shape, bool)
    if not len(rows) or away.all():
        return occ
    Nn, _ = ao.normals(g)
    o = hr.offset_ray(g["position"][..., :3].reshape(-1, 3)[rows], Nn[rows])
    o = np.repeat(o[:, None, :], away.shape[1], axis=1)[~away]
    with np.errstate(all="ignore"):
        wd = smp["Y"][~away] - o
        ln = np.sqrt(hr.dot(wd, wd))
        d = wd / ln[:, None]
        rays = np.zeros((len(o), 8), np.float32)
        rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.001, d, ln * F(0.999)
    _, mesh, _ = oracle.trace_closest(rays)
    occ[~away] = mesh != hr.MISS
    return occ


def clamp(x, cap):
    with np.errstate(all="ignore"):
        return np.minimum(np.where(x > 0, x, F(0.0)), F(cap)).astype(np.float32)


def mean(rec, cap):
    """(r_0 + r_1 + ... + r_{samples-1}) / (float)samples in sample order, then the clamp: (m, 3)"""
    acc = rec[:, 0].copy()
    for s in range(1, rec.shape[1]):
        acc = acc + rec[:, s]
    with np.errstate(all="ignore"):
        return clamp(acc / F(rec.shape[1]), cap)


def gather(oracle, meshes, g, view, params, tab):
    """the pass up to its filter: counts (H, W, 4) uint8, D and Sp (H, W, 3) float32, cast and emitter (H, W) bool, totals (pixels, samples,
    shadow_rays, occluded, emitter_pixels) and the samples' record with `occluded` (m, s) added"""
    Hh, Ww = g["position"].shape[:2]
    cast, emitter = classify(g, view, meshes, tab)
    smp = samples(g, view, meshes, params, tab)
    occ = verdicts(oracle, g, smp)
    smp["occluded"] = occ
    rows = smp["rows"]
    counts = np.zeros((Hh * Ww, 4), np.uint8)
    D, Sp = np.zeros((Hh * Ww, 3), np.float32), np.zeros((Hh * Ww, 3), np.float32)
    if len(rows):
        lit = ~smp["away"] & ~occ
        counts[rows, LIT], counts[rows, OCCLUDED], counts[rows, AWAY] = lit.sum(axis=1), occ.sum(axis=1), smp["away"].sum(axis=1)
        D[rows] = mean(np.where(lit[..., None], smp["d"], F(0.0)), params["max_radiance"])
        Sp[rows] = mean(np.where(lit[..., None], smp["s"], F(0.0)), params["max_radiance"])
    totals = (len(rows), len(rows) * int(params["samples"]), int((~smp["away"]).sum()), int(occ.sum()), int(emitter.sum()))
    return counts.reshape(Hh, Ww, 4), D.reshape(Hh, Ww, 3), Sp.reshape(Hh, Ww, 3), cast.reshape(Hh, Ww), emitter.reshape(Hh, Ww), totals, smp


def filter(g, E, cast, params):
    """(H, W, 4) float32, w = 1 where the pixel cast, else (0, 0, 0, 0). blur_radius 0: E. r > 0: the mean of E over the taps (dx, dy) in
    [-r, r]^2, dy outer, that lie in the frame, cast themselves and pass both thresholds against the centre; the centre always counts"""
    Hh, Ww = g["position"].shape[:2]
    Nn, _ = ao.normals(g)
    Nn, P = Nn.reshape(Hh, Ww, 3), g["position"][..., :3]
    r = int(params["blur_radius"])
    out = np.zeros((Hh, Ww, 4), np.float32)
    total, taps = np.zeros((Hh, Ww, 3), np.float32), np.zeros((Hh, Ww), np.uint32)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    ok = np.ones((Hh, Ww), bool)
                else:
                    Pt, Nt = gi._shifted(P, dx, dy, 0.0), gi._shifted(Nn, dx, dy, 0.0)
                    ok = gi._shifted(cast, dx, dy, False) & (hr.dot(Nt, Nn) >= F(params["blur_normal_cos"])) & (np.abs(hr.dot(Pt - P, Nn)) <= F(params["blur_plane"]))
                total = np.where(ok[..., None], total + gi._shifted(E, dx, dy, 0.0), total)
                taps += ok
        mean_ = total / taps.astype(np.float32)[..., None]
    out[..., :3] = np.where(cast[..., None], mean_, F(0.0))
    out[..., 3] = cast
    return out


def composite(g, deferred, Df, Spf, emitter, meshes, params):
    """deferred_output after the pass, from the deferred pass's own output: rgb += (((base / PI) Df) + Spf) intensity on the pixels that
    cast (Df.w == 1); the emitters' pixels become (1, 1, 1) * intensity with show_emitters; alpha untouched"""
    Hh, Ww = g["position"].shape[:2]
    A = g["albedo"].reshape(-1, 4)
    _, _, _, bc = materials(g, meshes)
    out = deferred.copy().reshape(-1, 4)
    D4, S4 = Df.reshape(-1, 4), Spf.reshape(-1, 4)
    with np.errstate(all="ignore"):
        base = fr.gamma_table()[A[:, :3]] * bc
        add = (((base / fr.PI) * D4[:, :3]) + S4[:, :3]) * F(params["intensity"])
        touched = D4[:, 3] != 0
        out[touched, :3] = out[touched, :3] + add[touched]
    if params["show_emitters"]:
        out[emitter.reshape(-1), :3] = F(1.0) * F(params["intensity"])
    return out.reshape(Hh, Ww, 4)


def image(oracle, meshes, g, view, params, deferred, tab=None):
    """the whole pass: dict(counts, diffuse, specular (H, W, 4), deferred (H, W, 4), cast, emitter, totals, samples)"""
    tab = table(meshes) if tab is None else tab
    counts, D, Sp, cast, emitter, totals, smp = gather(oracle, meshes, g, view, params, tab)
    Df, Spf = filter(g, D, cast, params), filter(g, Sp, cast, params)
    return dict(counts=counts, diffuse=Df, specular=Spf, deferred=composite(g, deferred, Df, Spf, emitter, meshes, params), cast=cast, emitter=emitter,
                totals=totals, samples=smp, table=tab, D=D, Sp=Sp)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
LAMP = dict(origin=(-1.0, 3.0, -1.5), eu=(2.0, 0.0, 0.0), ev=(0.0, 0.0, -1.5))  # a ceiling panel, y = 3, facing down
BOX = dict(centre=(0.0, 0.75, -0.6), half=(0.9, 0.75, 0.4))                      # its front face, z = -0.2, looks away from the lamp
CAMERA = ((0.3, 2.0, 4.0), (0.0, 0.8, -1.0), 60.0)


def _room(extra):
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box, quad

    floor = quad((-4.0, 0.0, 4.0), (8.0, 0.0, 0.0), (0.0, 0.0, -8.0), nu=2, nv=2)
    back = quad((-4.0, 0.0, -4.0), (8.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    lamp = quad(LAMP["origin"], LAMP["eu"], LAMP["ev"])
    meshes = [Mesh(*floor, rr.LAMBERTIAN, base_color=(0.8, 0.8, 0.8, 1.0)), Mesh(*back, rr.PBR, base_color=(0.9, 0.4, 0.3, 1.0), metallic=0.3, roughness=0.5),
              Mesh(*box(BOX["centre"], BOX["half"]), rr.LAMBERTIAN, base_color=(0.3, 0.7, 0.4, 1.0)),
              Mesh(*lamp, rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0))] + extra
    eye, target, fov = CAMERA
    return Scene("area_room", [(Model(meshes, []), None)], [], rr.camera.Camera(eye, target, fov, W / H, 0.01, 1000.0))


def room_scene():
    """scene 1: a floor, a back wall and a box under one ceiling quad (2 emitter triangles) toward the back of the room: the box shadows the
    floor before it, its front face looks away from the lamp, and the camera sees the lamp's underside"""
    return _room([])


SMALL_AREA = 1.49e-4  # the small emitter's one real triangle, against the lamp's triangles of 1.5: 10^4


def three_lamp_scene():
    """scene 2: the room with two more emitter meshes - a small one of one triangle 10^4 times smaller than the lamp, with a degenerate
    triangle (two corners the same) behind it in its index list, and a quad under a mirrored, rotated, non-uniformly scaled instance"""
    from rust_renderer_amd.scenes import Mesh, quad

    sv, si = quad((2.0, 1.0, -1.0), (0.02, 0.0, 0.0), (0.0, 0.0149, 0.0))
    si = np.concatenate([si[:3], np.array([si[0], si[0], si[1]], np.uint32)]).astype(np.uint32)  # one real triangle, one degenerate
    rot = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]], np.float32)
    mirrored = rr.transform3x4((-1.3, 0.8, 0.6), (-2.6, 1.6, -1.0), rot)
    mv, mi = quad((-0.1, -0.1, 0.0), (0.2, 0.0, 0.0), (0.0, 0.2, 0.0))
    return _room([Mesh(sv, si, rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0)), Mesh(mv, mi, rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0), transform=mirrored)])


def dark_scene():
    """scene 3: the room with the lamp a plain surface - no emitter"""
    s = _room([])
    s.models[0][0].meshes[3].material_type = rr.LAMBERTIAN
    s.name = "area_dark"
    return s


def open_floor_scene(half=(0.6, 0.4), height=1.5):
    """the known answer's scene: an open floor under one rectangular emitter parallel to it, centred over the origin"""
    from rust_renderer_amd.scenes import Mesh, Model, Scene, quad

    floor = quad((-6.0, 0.0, 6.0), (12.0, 0.0, 0.0), (0.0, 0.0, -12.0))
    lamp = quad((-half[0], height, half[1]), (2 * half[0], 0.0, 0.0), (0.0, 0.0, -2 * half[1]))
    meshes = [Mesh(*floor, rr.LAMBERTIAN, base_color=(0.8, 0.8, 0.8, 1.0)), Mesh(*lamp, rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0))]
    return Scene("area_open_floor", [(Model(meshes, []), None)], [], rr.camera.Camera((0.0, 1.2, 3.5), (0.0, 0.0, 0.0), 50.0, W / H, 0.01, 1000.0))


def scene_view(scene, width=W, height=H, **kw):
    """hybrid_util.frame_view"""
    v = scene.make_view(width, height, **kw)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    return v

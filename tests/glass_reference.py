"""CPU restatement of the ray-traced glass of the hybrid frame (uh_render_hybrid's UH_HYBRID_GLASS): which pixels cast, the event at an
interface (reference.rchit:62-79 without the draw), the first event at the G-buffer's surface, the two chains of every pixel walked
segment by segment, what a segment's end brings (the sky, an emitter, the next event, a cut, or the rtgi pass's shadowed-sun-lit Lambert),
the counts and events images, the pass's statistics and the composite, in numpy float32 in the order DESIGN.md section 2 "Ray-traced
glass" pins. The chain loop runs over tests/hybrid_reference.py's trace; the terminal radiance is composed from tests/rtgi_reference.py
(clamp, the scenes), tests/hybrid_reference.py (offset_ray, _uv, sample, the world-normal arithmetic), tests/hybrid_frame_reference.py
(light_records, PI) and the oracle's sky. Each function takes the G-buffer as an argument, so a test can feed it the device's own. With
the scenes the tests use. Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa
import rtao_reference as ao
import rtgi_reference as gi

F = np.float32
SUNLIT, DARK, EMITTER, MISSED = gi.SUNLIT, gi.DARK, gi.EMITTER, gi.MISSED
TIR, CUT0, CUT1 = 1, 2, 4  # the flag bits of an events texel's byte 2
W, H = gi.W, gi.H


def default_params(**kw):
    """uh_glass_default_params, with `kw` over it"""
    p = dict(max_events=8, max_radiance=16.0, intensity=1.0)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def iors(scene):
    """raytrace_properties.y of every mesh in upload order (hybrid_reference.upload_recorded keeps the type alone)"""
    return np.array([m.material_property for model, _ in scene.models for m in model.meshes], np.float32)


# ---- the event ------------------------------------------------------------------------------------------------------------------------
def schlick(cosine, ref_idx):
    """rchit:12-18"""
    r0 = (F(1.0) - ref_idx) / (F(1.0) + ref_idx)
    r0 = r0 * r0
    x = F(1.0) - cosine
    x5 = ((x * x) * (x * x)) * x
    return r0 + (F(1.0) - r0) * x5


def reflect(I, N):
    return I - N * (F(2.0) * hr.dot(N, I))[..., None]


def refract(I, N, eta):
    """GLSL refract: the zero vector where k < 0"""
    dn = hr.dot(N, I)
    k = F(1.0) - (eta * eta) * (F(1.0) - dn * dn)
    with np.errstate(invalid="ignore"):
        t = I * eta[..., None] - N * (eta * dn + np.sqrt(k))[..., None]
    return np.where((k < 0)[..., None], F(0.0), t).astype(np.float32)


def event(nd, N, ior):
    """Event(nd, N, ior) of (n, 3), (n, 3), (n,) float32: dict(R, T (n, 3), Fr, cos, sin, ratio (n,), cannot (n,) bool). N has been turned
    toward the ray where this is called, so dnd <= 0 and ratio = 1 / ior on the way out of the glass as on the way in: the reference's"""
    nd, N, ior = np.asarray(nd, np.float32), np.asarray(N, np.float32), np.asarray(ior, np.float32)
    with np.errstate(all="ignore"):
        dnd = hr.dot(nd, N)
        back = dnd > 0
        outward = np.where(back[:, None], -N, N)
        ratio = np.where(back, ior, F(1.0) / ior).astype(np.float32)
        cos = np.fmin(hr.dot(F(-1.0) * nd, outward), F(1.0))
        sin = np.sqrt(F(1.0) - cos * cos)
        cannot = ratio * sin > F(1.0)
        Fr = schlick(cos, ratio)
        R = reflect(nd, outward)
        T = refract(nd, outward, ratio)
    return dict(R=R.astype(np.float32), T=T, Fr=Fr.astype(np.float32), cos=cos, sin=sin, ratio=ratio, cannot=cannot)


def turn(N, d):
    """rchit:35-37: N turned toward the ray (-N where dot(N, d) > 0), and whether the turn took place"""
    with np.errstate(invalid="ignore"):
        flipped = hr.dot(N, d) > 0
    return np.where(flipped[:, None], -N, N).astype(np.float32), flipped


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------
def pixels(g, view, meshes, ior):
    """the pixels that cast: dict(rows (m,) into the flattened frame, P, Nf, I (m, 3), ior (m,)): RTGI's rule, a material in range and of
    type 2, I = normalize(P - eye) finite; Nf = dot(Nn, I) > 0 ? -Nn : Nn"""
    Nn, geo = ao.normals(g)
    R = g["pbr"].reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        material = R[:, 3].astype(np.uint32)
    valid = material < len(meshes)
    idx = np.where(valid, material, 0)
    typ = np.where(valid, np.array([m["type"] for m in meshes] or [0.0], np.float32)[idx], F(0.0))
    P = g["position"][..., :3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        I = hr.normalize(P - np.array(view.eye_pos[:3], np.float32)[None, :])
        cast = geo & (typ == 2.0) & np.isfinite(I).all(axis=1)
        rows = np.nonzero(cast)[0]
        i = I[rows]
        Nf, _ = turn(Nn[rows], i)
    return dict(rows=rows, P=P[rows], Nf=Nf.astype(np.float32), I=i, ior=np.asarray(ior, np.float32)[idx[rows]] if len(rows) else np.zeros(0, np.float32))


def hit_normals(meshes, mesh, prim, u, v, d):
    """rchit:30-37 of the hits (mesh, prim, u, v) of rays with direction d: Nh turned toward the ray, and whether the turn took place"""
    b0, b1, b2 = (F(1.0) - u) - v, u, v
    Nh = np.zeros((len(mesh), 3), np.float32)
    with np.errstate(all="ignore"):
        for i in np.unique(mesh):
            sel = mesh == i
            M = meshes[int(i)]
            tri = M["indices"].reshape(-1, 3)[prim[sel]]
            vn = [M["vertices"]["normal"][tri[:, k], :3].astype(np.float32) for k in range(3)]
            n = (vn[0] * b0[sel][:, None] + vn[1] * b1[sel][:, None]) + vn[2] * b2[sel][:, None]
            Nh[sel] = hr.normalize(hr.inverse_transpose_mul(hr.invert3x3(M["world"]), n))
        return turn(Nh, d)


def lambert(oracle, meshes, view, o, d, t, u, v, mesh, prim):
    """the rtgi pass's Lambert lines (rtgi_reference.rays, word for word) for hits of rays (o, d) on meshes of no special type: L before
    the clamp (0 where dark), whether a sun ray was cast and whether it was occluded"""
    n = len(mesh)
    L = np.zeros((n, 3), np.float32)
    cast_sun, occluded = np.zeros(n, bool), np.zeros(n, bool)
    if not n:
        return L, cast_sun, occluded
    with np.errstate(all="ignore"):
        b0, b1, b2 = (F(1.0) - u) - v, u, v
        uu, vv = hr._uv(meshes, mesh, prim, b0, b1, b2)
        tex = hr.sample(oracle, np.array([meshes[int(i)]["diffuse_map"] for i in mesh], np.uint32), uu, vv)
        albedo = tex * np.array([meshes[int(i)]["base_color"] for i in mesh], np.float32).reshape(-1, 3)  # rchit:41-42
        Nh, _ = hit_normals(meshes, mesh, prim, u, v, d)
        X = o + t[:, None] * d
        sun = hr.sun_direction(view)
        ndl = hr.dot(Nh, np.broadcast_to(sun, Nh.shape))
        NdotL = np.where(ndl > 0, ndl, F(0.0))  # max(dot, 0); a NaN is 0
        ci = np.nonzero(NdotL > 0)[0]
        _, _, _, blocker, _ = hr.trace(oracle, hr.offset_ray(X[ci], Nh[ci]), np.broadcast_to(sun, (len(ci), 3)))
        rad_sun = fr.light_records(view, [])[0]["color"] * F(1.0)
        L[ci] = ((albedo[ci] / fr.PI) * rad_sun[None, :]) * NdotL[ci][:, None]
        cast_sun[ci] = True
        occluded[ci] = blocker != hr.MISS
    return L, cast_sun, occluded


def chains(oracle, meshes, ior, g, view, params, furnace=False):
    """both chains of every pixel that casts, walked in rounds as the pass walks them. dict(px (pixels()), R (m, 2, 3): the records w L as
    stored, kind (m, 2) of SUNLIT / DARK / EMITTER / MISSED, events (m, 2) (0: not cast), cut (m, 2), tir0 (m,): first-event TIR,
    shadowed (m, 2): dark because its sun ray was occluded, weights (m, 2), first (event() of the first event), rounds: the rays of each
    round, backface (m, 2): per chain, the events at a hit whose normal was turned, as a list of the meshes they took place on, and
    totals: dict of UhGlassStats' integers)"""
    px = pixels(g, view, meshes, ior)
    ior = np.asarray(ior, np.float32)
    m, cap, top = len(px["rows"]), F(params["max_radiance"]), int(params["max_events"])
    n = 2 * m
    first = event(px["I"], px["Nf"], px["ior"])
    tir0 = first["cannot"].copy()
    w = np.zeros(n, np.float32)
    w[0::2] = np.where(tir0, F(1.0), first["Fr"])
    w[1::2] = F(1.0) - first["Fr"]
    o = np.repeat(hr.offset_ray(px["P"], px["Nf"]), 2, axis=0).astype(np.float32) if m else np.zeros((0, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    d[0::2], d[1::2] = first["R"], first["T"]
    events = np.ones(n, np.uint32)
    events[1::2][tir0] = 0
    R = np.zeros((n, 3), np.float32)
    kind = np.full(n, DARK, np.uint8)
    cut, shadowed = np.zeros(n, bool), np.zeros(n, bool)
    backface = [[] for _ in range(n)]
    active = np.nonzero(events > 0)[0]
    totals = dict(pixels=m, chains=len(active), segments=0, events=0, tir=int(tir0.sum()), cut=0, shadow_rays=0, misses=0)
    rounds = []
    types = np.array([M["type"] for M in meshes], np.float32)
    for _ in range(top):
        rounds.append(len(active))
        totals["segments"] += len(active)
        if not len(active):
            continue
        oo, dd = o[active], d[active]
        t, u, v, mesh, prim = hr.trace(oracle, oo, dd)
        L = np.zeros((len(active), 3), np.float32)
        ends = np.ones(len(active), bool)
        miss = mesh == hr.MISS
        kind[active[miss]] = MISSED
        totals["misses"] += int(miss.sum())
        for k in np.nonzero(miss)[0]:
            L[k] = 1.0 if furnace else oa.sky(oo[k], dd[k], view.sun_dir[:])
        ty = np.where(miss, F(-1.0), types[np.where(miss, 0, mesh)])
        emit = ty == 3.0
        kind[active[emit]] = EMITTER
        L[emit] = 1.0
        glass = np.nonzero(ty == 2.0)[0]
        capped = events[active[glass]] == top
        cut[active[glass[capped]]] = True
        bend = glass[~capped]
        if len(bend):
            Nh, flipped = hit_normals(meshes, mesh[bend], prim[bend], u[bend], v[bend], dd[bend])
            e = event(hr.normalize(dd[bend]), Nh, ior[mesh[bend]])
            totals["tir"] += int(e["cannot"].sum())
            dn = np.where(e["cannot"][:, None], e["R"], e["T"]).astype(np.float32)
            with np.errstate(all="ignore"):
                bad = ~np.isfinite(dn).all(axis=1) | (hr.dot(dn, dn) == 0)
                X = oo[bend] + t[bend][:, None] * dd[bend]
            cut[active[bend[bad]]] = True
            go = bend[~bad]
            ends[go] = False
            o[active[go]] = hr.offset_ray(X[~bad], Nh[~bad])
            d[active[go]] = dn[~bad]
            events[active[go]] += 1
            totals["events"] += len(go)
            for k, f, mi in zip(active[bend], flipped, mesh[bend]):
                if f:
                    backface[k].append(int(mi))
        rest = np.nonzero((ty >= 0) & (ty != 3.0) & (ty != 2.0))[0]
        if len(rest) and not furnace:
            Lr, cast_sun, occluded = lambert(oracle, meshes, view, oo[rest], dd[rest], t[rest], u[rest], v[rest], mesh[rest], prim[rest])
            L[rest] = Lr
            kind[active[rest[cast_sun & ~occluded]]] = SUNLIT
            shadowed[active[rest[occluded]]] = True
            L[rest[occluded]] = 0.0  # the sun ray zeroes the record
            totals["shadow_rays"] += int(cast_sun.sum())
        done = active[ends]
        with np.errstate(all="ignore"):
            R[done] = w[done][:, None] * gi.clamp(L[ends], cap)
        active = active[~ends]
    assert not len(active), "max_events rounds end every chain"
    totals["cut"] = int(cut.sum())
    shape = lambda a: a.reshape(m, 2, *a.shape[1:])
    return dict(px=px, R=shape(R), kind=shape(kind), events=shape(events), cut=shape(cut), tir0=tir0, shadowed=shape(shadowed), weights=shape(w), first=first,
                rounds=rounds, backface=[backface[2 * q:2 * q + 2] for q in range(m)], totals=totals)


def clamp_sum(ch, max_radiance):
    """C = clamp(R_0 + R_1) per channel of every pixel that cast: (m, 3)"""
    with np.errstate(all="ignore"):
        return gi.clamp(ch["R"][:, 0] + ch["R"][:, 1], max_radiance)


def images(g, ch, params):
    """UH_HYBRID_GLASS_RADIANCE (H, W, 4) float32, UH_HYBRID_GLASS_COUNTS and UH_HYBRID_GLASS_EVENTS (H, W, 4) uint8, and the pixels that
    cast (H, W) and those with a missed chain (H, W), from chains()'s dict: C = clamp(R_0 + R_1)"""
    Hh, Ww = g["position"].shape[:2]
    rows = ch["px"]["rows"]
    radiance = np.zeros((Hh * Ww, 4), np.float32)
    counts, ev = np.zeros((Hh * Ww, 4), np.uint8), np.zeros((Hh * Ww, 4), np.uint8)
    cast, missed = np.zeros(Hh * Ww, bool), np.zeros(Hh * Ww, bool)
    if len(rows):
        cast[rows] = True
        radiance[rows, :3] = clamp_sum(ch, params["max_radiance"])
        radiance[rows, 3] = 1.0
        for k in range(4):
            counts[rows, k] = (ch["kind"] == k).sum(axis=1)
        ev[rows, 0], ev[rows, 1] = ch["events"][:, 0], ch["events"][:, 1]
        ev[rows, 2] = ch["tir0"] * TIR + ch["cut"][:, 0] * CUT0 + ch["cut"][:, 1] * CUT1
        missed[rows] = (ch["kind"] == MISSED).any(axis=1)
    shape = lambda a: a.reshape(Hh, Ww, *a.shape[1:])
    return shape(radiance), shape(counts), shape(ev), shape(cast), shape(missed)


def composite(deferred, radiance, intensity):
    """deferred_output after the pass, from the output it replaces: rgb = C * intensity where the pixel cast; alpha untouched"""
    out = deferred.copy()
    cast = radiance[..., 3] != 0
    with np.errstate(all="ignore"):
        out[cast, :3] = radiance[cast, :3] * F(intensity)
    return out


def cpu_world(scene, width=W, height=H):
    """the scene on the oracle alone: (oracle, meshes as add_mesh received them, iors, the view, the oracle's G-buffer)"""
    cpu = oa.OracleRenderer(width, height)
    meshes = hr.upload_recorded(scene, cpu, True)
    v = scene_view(scene, width, height)
    return cpu, meshes, iors(scene), v, hr.gbuffer(cpu, meshes, v, width, height)


def classes(ch, ch2, mirrored):
    """the pixel counts the gallery's adequacy is stated in, from chains() at the tested max_events (ch) and at max_events = 2 (ch2);
    mirrored: the index of the mesh under the mirrored transform"""
    ev, kind = ch["events"], ch["kind"]
    return dict(first_event_tir=int(ch["tir0"].sum()),
                chain1_two_events=int((ev[:, 1] == 2).sum()),
                four_or_more_events=int((ev >= 4).any(axis=1).sum()),
                cut_at_two=int(ch2["cut"].any(axis=1).sum()),
                sunlit=int((kind == SUNLIT).any(axis=1).sum()),
                shadowed=int(ch["shadowed"].any(axis=1).sum()),
                emitter=int((kind == EMITTER).any(axis=1).sum()),
                missed=int((kind == MISSED).any(axis=1).sum()),
                backface_on_mirrored=int(sum(any(mirrored in c for c in pair) for pair in ch["backface"])))


def assert_adequate(ch, ch2):
    """at least 100 pixels in every class, and at least half of the casting pixels without a missed chain"""
    got = classes(ch, ch2, GALLERY_MESHES["mirrored"])
    assert min(got.values()) >= 100, got
    m = len(ch["px"]["rows"])
    assert 2 * got["missed"] <= m, (got["missed"], m)
    return got


def integers(s):
    """UhGlassStats' integers as chains()'s totals name them"""
    return dict(pixels=s.pixels, chains=s.chains, segments=s.segments, events=s.events, tir=s.tir, cut=s.cut, shadow_rays=s.shadow_rays, misses=s.misses)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
GALLERY_SUN = (0.1, 0.9, 0.3)  # toward the sun: steeply through the canopy's opening onto the middle of the floor
GALLERY_MESHES = dict(floor=0, back=1, sides=2, canopy=3, block=4, ball=5, slab=6, thin=7, far_ball=8, mirrored=9, lamp=10, metal=11)
GALLERY_SIZE = (2 * W, 2 * H)  # 134 x 82: the frame of the gallery's tests; at 67 x 41 only 65 pixels have a chain that ends sunlit


def gallery_scene():
    """rtgi_reference's courtyard with glass in it: an ior-1.5 ball and a larger one behind it as the camera sees them (a chain through both
    has four events and more), an ior-1.5 slab standing before the red wall - the sunlit foot of the wall, the lamp and the wall's
    shadowed part show through it, and the sun rays of the wall behind it meet it -, an ior-0.6 slab lying on the floor, whose top the
    camera sees at more than asin(0.6) from its normal (first-event TIR), a glass box under a mirrored, rotated and non-uniformly scaled
    instance, a type-3 lamp on the back wall and a type-1 metal ball"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box, icosphere, quad

    yard = gi.courtyard_scene()
    meshes = list(yard.models[0][0].meshes)
    sv, si = icosphere(2)
    rot = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]], np.float32)
    glass = lambda vi, ior, **kw: Mesh(*vi, rr.DIELECTRIC, ior, base_color=(1.0, 1.0, 1.0, 1.0), **kw)
    meshes += [glass((sv, si), 1.5, transform=rr.transform3x4((0.45, 0.45, 0.45), (0.8, 1.0, 0.9))),
               glass(box((-0.5, 0.7, 0.3), (0.8, 0.6, 0.06)), 1.5),
               glass(box((0.5, 0.8, 1.7), (0.8, 0.08, 0.5)), 0.6),
               glass((sv, si), 1.5, transform=rr.transform3x4((0.8, 0.8, 0.8), (1.1, 0.8, -1.4))),
               glass(box((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)), 1.5, transform=rr.transform3x4((-0.7, 0.9, 0.5), (-1.8, 0.6, 0.6), rot)),
               Mesh(*quad((-2.5, 0.1, -2.97), (4.0, 0.0, 0.0), (0.0, 1.6, 0.0)), rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0)),
               Mesh(sv, si, rr.METAL, 0.1, base_color=(0.9, 0.6, 0.3, 1.0), transform=rr.transform3x4((0.35, 0.35, 0.35), (-2.3, 0.35, -1.0)))]
    return Scene("glass_gallery", [(Model(meshes, [gi.checker()]), None)], [], yard.camera)


def nested_boxes_scene():
    """the camera inside a glass box, inside a second glass box, inside rtgi_reference's box with every wall of material type 3: every
    pixel casts, every chain ends at the emitter (chain 1 after 2 events, chain 0 after 3), no sky integral"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box

    cam = rr.camera.Camera((0.1, 1.05, 0.6), (0.0, 1.0, -1.2), 30.0, W / H, 0.01, 1000.0)
    meshes = [Mesh(*box((0.1, 1.05, 0.5), (0.3, 0.3, 0.4)), rr.DIELECTRIC, 1.5), Mesh(*box((0.0, 1.0, 0.0), (0.7, 0.55, 0.95)), rr.DIELECTRIC, 1.5),
              Mesh(*gi._inward_walls(), rr.DIFFUSE_LIGHT, base_color=(1.0, 1.0, 1.0, 1.0))]
    return Scene("glass_nested_boxes", [(Model(meshes, []), None)], [], cam)


def no_glass_scene():
    """rtgi_reference's courtyard as it is: no pixel casts"""
    return gi.courtyard_scene()


WALK_LANES = gi.WALK_LANES
WALK_NESTED_SIZE = (263, 167)  # the nested boxes: 87,842 rays in round 0 and in round 1, more than WALK_LANES: both queues refill


def scene_view(scene, width=W, height=H, **kw):
    """rtgi_reference.scene_view; the gallery has the courtyard's sun"""
    v = gi.scene_view(scene, width, height, **kw)
    if scene.name == "glass_gallery":
        s = np.array(GALLERY_SUN, np.float64)
        v.sun_dir[:] = [float(x) for x in np.float32(s / np.linalg.norm(s))]
    return v

"""CPU restatement of ray-traced ambient occlusion (uh_render_hybrid's UH_HYBRID_RTAO): which pixels cast, their cosine-weighted hemisphere
rays, the occluded-ray counts and the resolve / filter that writes ssao_output, in numpy float32 in the order DESIGN.md section 2
"Ray-traced ambient occlusion" pins. Composed from tests/hybrid_reference.py (offset_ray, normalize, trace through the oracle's
trace_closest with the predicate "hit and t <= radius", as hybrid_restir_reference.occluded) and the oracle's init_rng,
random_point_in_unit_sphere and frame_number. Each function takes the G-buffer as an argument, so a test can feed it the device's own.
Not a conftest: test modules import it."""
import functools

import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import oracle_api as oa

F = np.float32
MAX_SAMPLES = 64


def default_params(**kw):
    """uh_rtao_default_params, with `kw` over it"""
    p = dict(samples=4, radius=1.0, strength=1.0, blur_radius=2, blur_normal_cos=0.9, blur_plane=0.05)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def normals(g):
    """Nn = normalize(N) of every pixel (n, 3) and which pixels cast: geometry (position w != 0) with Nn finite"""
    P4 = g["position"].reshape(-1, 4)
    Nn = hr.normalize(g["normal"][..., :3].reshape(-1, 3))
    return Nn, (P4[:, 3] != 0) & np.isfinite(Nn).all(axis=1)


@functools.lru_cache(maxsize=None)
def _sphere_points(W, H, frame, s):
    """randomPointInUnitSphere of the state initRNG(px, py, W, frame * 64 + s) for every pixel of a W x H frame: (H * W, 3)"""
    out = np.empty((W * H, 3), np.float32)
    f = (frame * MAX_SAMPLES + s) & 0xFFFFFFFF
    for pix in range(W * H):
        out[pix], _ = oa.random_point_in_unit_sphere(oa.init_rng(pix % W, pix // W, W, f))
    out.setflags(write=False)
    return out


def directions(g, view, samples):
    """the pixels that cast (indices into the flattened frame), their Nn (m, 3), and the ray directions (m, samples, 3):
    d = normalize(Nn + normalize(u)), Nn itself where |Nn + normalize(u)|^2 is not >= 1e-12"""
    H, W = g["position"].shape[:2]
    Nn, cast = normals(g)
    rows = np.nonzero(cast)[0]
    frame = oa.frame_number(view)
    nn = Nn[rows]
    d = np.empty((len(rows), samples, 3), np.float32)
    with np.errstate(all="ignore"):
        for s in range(samples):
            u = hr.normalize(_sphere_points(W, H, frame, s)[rows])
            w = nn + u
            d[:, s] = np.where((hr.dot(w, w) >= F(1e-12))[:, None], hr.normalize(w), nn)
    return rows, nn, d


def occluded(oracle, o, d, radius):
    """some triangle has 0.001 < t < 10000 and t <= radius: the closest hit decides"""
    t, _, _, mesh, _ = hr.trace(oracle, o, d)
    return (mesh != hr.MISS) & (t <= F(radius))


def counts(oracle, g, view, samples, radius):
    """the occluded-ray counts (H, W) uint8 in G-buffer orientation, and the pass's totals (pixels, rays, occluded)"""
    H, W = g["position"].shape[:2]
    rows, nn, d = directions(g, view, samples)
    out = np.zeros(H * W, np.uint8)
    if len(rows):
        o = hr.offset_ray(g["position"][..., :3].reshape(-1, 3)[rows], nn)
        occ = occluded(oracle, np.repeat(o, samples, axis=0), d.reshape(-1, 3), radius).reshape(len(rows), samples)
        out[rows] = occ.sum(axis=1)
    return out.reshape(H, W), (len(rows), len(rows) * samples, int(out.sum()))


def ao_raw(count, samples, strength):
    """1 - strength * ((float)count / (float)samples)"""
    return F(1.0) - F(strength) * (count.astype(np.float32) / F(samples))


def resolve(g, count, samples, strength, blur_radius=0, blur_normal_cos=0.9, blur_plane=0.05):
    """ssao_output (H, W) uint16 from the counts: texel (x, y) belongs to G-buffer pixel (x, H - 1 - y). A pixel that cast nothing is
    65535. blur_radius r > 0: the mean of ao_raw over the taps (dx, dy) in [-r, r)^2, dy outer, that lie in the frame, cast themselves
    and pass both thresholds against the centre; the centre always counts; float32 sum in that order, divided by the tap count."""
    H, W = g["position"].shape[:2]
    Nn, cast = normals(g)
    cast = cast.reshape(H, W)
    raw = ao_raw(count, samples, strength)
    if blur_radius == 0:
        return np.where(cast, fr.unorm16(raw), 65535).astype(np.uint16)[::-1]
    r = int(blur_radius)
    P, Nn = g["position"][..., :3], Nn.reshape(H, W, 3)

    def shifted(a, dx, dy, fill):
        """a[y + dy, x + dx] where that lies in the frame, else fill"""
        out = np.full_like(a, fill)
        if abs(dx) >= W or abs(dy) >= H:
            return out
        ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
        xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
        out[yd, xd] = a[ys, xs]
        return out

    total, taps = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32)
    with np.errstate(all="ignore"):
        for dy in range(-r, r):
            for dx in range(-r, r):
                if dx == 0 and dy == 0:
                    ok = np.ones((H, W), bool)
                else:
                    Pt, Nt = shifted(P, dx, dy, 0.0), shifted(Nn, dx, dy, 0.0)
                    ok = shifted(cast, dx, dy, False) & (hr.dot(Nt, Nn) >= F(blur_normal_cos)) & (np.abs(hr.dot(Pt - P, Nn)) <= F(blur_plane))
                total = np.where(ok, total + shifted(raw, dx, dy, 0.0), total)
                taps += ok
        out = fr.unorm16(total / taps.astype(np.float32))
    return np.where(cast, out, 65535).astype(np.uint16)[::-1]


def image(oracle, g, view, params):
    """counts, totals and ssao_output of one pass with `params` (a dict as default_params makes it)"""
    count, totals = counts(oracle, g, view, params["samples"], params["radius"])
    img = resolve(g, count, params["samples"], params["strength"], params["blur_radius"], params["blur_normal_cos"], params["blur_plane"])
    return count, totals, img


# ---- scenes with known answers ---------------------------------------------------------------------------------------------------
W, H = 67, 41
BOX_CENTRE, BOX_HALF = (0.0, 1.0, 0.0), (1.0, 0.8, 1.2)
BOX_RADIUS = 4.0  # above the box's diagonal, 2 |BOX_HALF| = 3.51: whatever a ray inside the box meets, it meets within the radius


def floor_scene():
    """a bare floor of two triangles: no hemisphere ray from it meets anything"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, quad

    fv, fi = quad((-23.0, 0.0, 19.0), (41.0, 0.0, 0.0), (0.0, 0.0, -43.0))
    cam = rr.camera.Camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), 60.0, W / H, 0.01, 1000.0)
    return Scene("rtao_floor", [(Model([Mesh(fv, fi, rr.LAMBERTIAN, base_color=(0.8, 0.7, 0.6, 1.0))], []), None)], [], cam)


def inward_box_scene():
    """the camera inside a closed box whose vertex normals point inward (scenes.box with the normals negated; the triangle test culls
    nothing, so the winding does not matter), looking at the middle of one wall through a narrow lens: every pixel is that wall, no
    pixel lies within the rays' tmin (0.001) of an edge - a ray from such a pixel toward the adjacent wall would start behind its hit -
    and every ray meets another wall within BOX_RADIUS. Checked on the restatement alone (test_rtao_cpu.py) at 67 x 41 with 8 samples: no
    ray leaks through an edge. (A camera that sees the box's edges does leak there: 3 of 21,976 rays, all from pixels less than
    0.001 from an edge.)"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, box

    bv, bi = box(BOX_CENTRE, BOX_HALF)
    bv["normal"][:, :3] *= -1.0
    cam = rr.camera.Camera((0.1, 1.05, 0.6), (0.0, 1.0, -1.2), 30.0, W / H, 0.01, 1000.0)
    return Scene("rtao_inward_box", [(Model([Mesh(bv, bi, rr.LAMBERTIAN, base_color=(0.7, 0.7, 0.8, 1.0))], []), None)], [], cam)

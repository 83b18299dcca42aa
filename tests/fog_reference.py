"""CPU restatement of the volumetric fog pass (uh_render_hybrid's UH_HYBRID_FOG): which pixels march, their samples' sun rays and the bit
masks they leave, the resolve (a, Ttot, F), the depth-stopped filter (Ff), the Henyey-Greenstein phase and the composite, in numpy float32
in the order DESIGN.md section 2 "Volumetric fog" pins. Composed from tests/hybrid_reference.py (trace through the oracle's trace_closest,
dot, sun_direction), tests/taa_reference.py (the primary rays) and the oracle's init_rng, random_floats and frame_number. Each function
takes the G-buffer and deferred_output as arguments, so a test can feed it the device's own. Also the scenes with known answers and the
float64 predicate of the slab scene's shafts. Not a conftest: test modules import it."""
import functools

import numpy as np

import hybrid_reference as hr
import oracle_api as oa
import taa_reference as tr

F = np.float32
SEED_XOR = 0x464F4721
PI = F(3.14159265359)  # brdf.glsl:1
RAD_SUN = F(1.0) * F(1.0)  # the deferred pass's light record 0: color (1, 1, 1) times attenuation 1, as the rtgi pass takes it
W, H = 67, 41


def default_params(**kw):
    """uh_fog_default_params, with `kw` over it"""
    p = dict(steps=16, blur_radius=2, density=0.02, max_distance=200.0, anisotropy=0.6, intensity=1.0, blur_depth=0.1, albedo=(1.0, 1.0, 1.0),
             ambient=(0.05, 0.06, 0.08))
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def rays(position, view, max_distance):
    """the marches of a frame: o (3,), dir (n, 3), D (n,) (0 where the pixel does not march) and which pixels march (n,)"""
    Hh, Ww = position.shape[:2]
    iv = np.array(view.inverse_view[:], np.float32)
    o = np.array(tr.mat4_mul(iv, F(0.0), F(0.0), F(0.0), F(1.0))[:3], np.float32)
    d = tr.primary_directions(view, Ww, Hh)
    P4 = position.reshape(-1, 4)
    geo = P4[:, 3] != 0
    with np.errstate(all="ignore"):
        V = P4[:, :3] - o
        D0 = np.sqrt(hr.dot(V, V))
        ok = np.isfinite(D0) & (D0 > 0)
        towards = V / D0[:, None]
        marched = ~geo | ok
        direction = np.where(geo[:, None], towards, d)
        D = np.where(geo, np.minimum(D0, F(max_distance)), F(max_distance))
    return o, direction, np.where(marched, D, F(0.0)).astype(np.float32), marched


@functools.lru_cache(maxsize=None)
def _jitter(Ww, Hh, frame):
    """xi = randomFloat of the state initRNG(px, py, W, (frame * 64) ^ SEED_XOR) for every pixel: (H * W,)"""
    seed = ((frame * 64) & 0xFFFFFFFF) ^ SEED_XOR
    out = np.empty(Ww * Hh, np.float32)
    for pix in range(Ww * Hh):
        out[pix] = oa.random_floats(oa.init_rng(pix % Ww, pix // Ww, Ww, seed), 1)[0][0]
    out.setflags(write=False)
    return out


def sample_points(position, view, steps, max_distance):
    """the pixels that march (indices into the flattened frame) and X_k = o + dir * (((float)k + xi) * dt): (m, steps, 3)"""
    Hh, Ww = position.shape[:2]
    o, direction, D, marched = rays(position, view, max_distance)
    rows = np.nonzero(marched)[0]
    dt = D[rows] / F(steps)
    xi = _jitter(Ww, Hh, oa.frame_number(view))[rows]
    X = np.empty((len(rows), steps, 3), np.float32)
    for k in range(steps):
        X[:, k] = o + direction[rows] * ((F(k) + xi) * dt)[:, None]
    return rows, X


def masks(oracle, position, view, steps, max_distance):
    """the masks (H, W) uint32 in G-buffer orientation - bit k: the any-hit ray of sample k toward the sun (tmin 0.001, tmax 10000) is
    not occluded - and the pass's totals (pixels, rays, lit)"""
    Hh, Ww = position.shape[:2]
    rows, X = sample_points(position, view, steps, max_distance)
    out = np.zeros(Hh * Ww, np.uint32)
    if len(rows):
        sun = hr.sun_direction(view)
        _, _, _, mesh, _ = hr.trace(oracle, X.reshape(-1, 3), np.broadcast_to(sun, (len(rows) * steps, 3)))
        lit = (mesh == hr.MISS).reshape(len(rows), steps)
        out[rows] = (lit.astype(np.uint32) << np.arange(steps, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
    return out.reshape(Hh, Ww), (len(rows), len(rows) * steps, int(sum(bin(int(m)).count("1") for m in out[rows])))


def attenuation(D, steps, density):
    """a = expf(-(density * dt)) with dt = D / (float)steps"""
    return np.exp(-(F(density) * (D / F(steps)))).astype(np.float32)


def resolve(mask, D, marched, steps, density, a=None):
    """(a, Ttot, F) of every pixel (n,), all 0 where it did not march: p = 1, sum = 0; for k: if bit k: sum += p; p = p * a; Ttot = p,
    F = (1 - a) * sum. `a`: the device's own, or None for numpy's exp"""
    mask = mask.reshape(-1)
    if a is None:
        a = attenuation(D, steps, density)
    a = np.asarray(a, np.float32).reshape(-1)
    p, total = np.ones_like(a), np.zeros_like(a)
    for k in range(steps):
        total = np.where((mask >> np.uint32(k)) & np.uint32(1) != 0, total + p, total)
        p = p * a
    zero = F(0.0)
    return np.where(marched, a, zero), np.where(marched, p, zero), np.where(marched, (F(1.0) - a) * total, zero)


def blur(Fr, D, marched, Ww, Hh, r, blur_depth):
    """Ff (n,): r == 0: F. Else the float32 sum of F over the taps (dx, dy) in [-r, r]^2, dy outer, that lie in the frame, marched and
    have |D_tap - D| <= blur_depth * D (the centre always counts), divided by the float tap count; 0 where the pixel did not march"""
    if r == 0:
        return Fr.copy()
    Fi, Di, Mi = Fr.reshape(Hh, Ww), D.reshape(Hh, Ww), marched.reshape(Hh, Ww)
    y, x = np.mgrid[0:Hh, 0:Ww]
    total, taps = np.zeros((Hh, Ww), np.float32), np.zeros((Hh, Ww), np.float32)
    bound = F(blur_depth) * Di
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            qx, qy = x + dx, y + dy
            inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
            cx, cy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
            if dx == 0 and dy == 0:
                ok = np.ones((Hh, Ww), bool)
            else:
                ok = inside & Mi[cy, cx] & (np.abs(Di[cy, cx] - Di) <= bound)
            total = np.where(ok, total + Fi[cy, cx], total)
            taps = np.where(ok, taps + F(1.0), taps)
    return np.where(Mi, total / taps, F(0.0)).reshape(-1).astype(np.float32)


def phase(sun, direction, g):
    """Henyey-Greenstein without pow: q = (1 + g g) - (2 g) c, ph = (1 - g g) / ((4 PI) * (q * sqrt(q)))"""
    g = F(g)
    c = hr.dot(np.broadcast_to(np.asarray(sun, np.float32), direction.shape), direction)
    q = (F(1.0) + g * g) - (F(2.0) * g) * c
    with np.errstate(all="ignore"):
        return (F(1.0) - g * g) / ((F(4.0) * PI) * (q * np.sqrt(q)))


def composite(deferred, marched, Ttot, Ff, ph, params):
    """out = (C * Ttot + S * Ff) + ambient * (1 - Ttot) on the pixels that marched, S = ((albedo * rad_sun) * ph) * intensity; alpha and
    every other pixel untouched. deferred (H, W, 4)"""
    out = deferred.reshape(-1, 4).copy()
    albedo, ambient = np.array(params["albedo"], np.float32), np.array(params["ambient"], np.float32)
    with np.errstate(all="ignore"):
        S = ((albedo * RAD_SUN)[None, :] * ph[:, None]) * F(params["intensity"])
        C = out[:, :3]
        fogged = (C * Ttot[:, None] + S * Ff[:, None]) + ambient[None, :] * (F(1.0) - Ttot)[:, None]
    out[:, :3] = np.where(marched[:, None], fogged, C)
    return out.reshape(deferred.shape)


def shade(mask, position, deferred, view, params, a=None):
    """what follows the walk, from the masks: the terms image (H, W, 4) (a, Ttot, F, Ff) and the fogged deferred_output"""
    Hh, Ww = position.shape[:2]
    _, direction, D, marched = rays(position, view, params["max_distance"])
    a, Ttot, Fr = resolve(mask, D, marched, params["steps"], params["density"], a)
    Ff = blur(Fr, D, marched, Ww, Hh, int(params["blur_radius"]), params["blur_depth"])
    ph = phase(hr.sun_direction(view), direction, params["anisotropy"])
    terms = np.stack([a, Ttot, Fr, Ff], axis=-1).astype(np.float32).reshape(Hh, Ww, 4)
    return terms, composite(deferred, marched, Ttot, Ff, ph, params)


# ---- scenes with known answers ---------------------------------------------------------------------------------------------------
SLAB_Y, SLAB_HALF, HOLE_HALF = 4.0, 20.0, 1.0
SLAB_SUN = (0.35, 1.0, 0.2)         # toward the sun, at a slant
SLAB_MAX_DISTANCE = 14.0            # every sample stays well inside the slab's span
BOUNDARY = 1e-3                     # samples closer than this to a shadow boundary or to the slab are not compared


def floor_scene():
    """a bare floor of two triangles under the default sun: no sun ray meets anything"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, quad

    fv, fi = quad((-23.0, 0.0, 19.0), (41.0, 0.0, 0.0), (0.0, 0.0, -43.0))
    cam = rr.camera.Camera((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), 60.0, W / H, 0.01, 1000.0)
    return Scene("fog_floor", [(Model([Mesh(fv, fi, rr.LAMBERTIAN, base_color=(0.8, 0.7, 0.6, 1.0))], []), None)], [], cam)


def slab_scene(width=W, height=H):
    """a floor at y = 0 and a sheet at y = SLAB_Y spanning +-SLAB_HALF with a hole of +-HOLE_HALF around the origin, four quads; the camera
    under the sheet looks across the column of light the hole lets in (view it with slab_view: the sun at a slant)"""
    import rust_renderer_amd as rr
    from rust_renderer_amd.scenes import Mesh, Model, Scene, quad

    s, h, y = SLAB_HALF, HOLE_HALF, SLAB_Y
    parts = [quad((-30.0, 0.0, 30.0), (60.0, 0.0, 0.0), (0.0, 0.0, -60.0)),
             quad((-s, y, s), (s - h, 0.0, 0.0), (0.0, 0.0, -2 * s)), quad((h, y, s), (s - h, 0.0, 0.0), (0.0, 0.0, -2 * s)),
             quad((-h, y, s), (2 * h, 0.0, 0.0), (0.0, 0.0, -(s - h))), quad((-h, y, -h), (2 * h, 0.0, 0.0), (0.0, 0.0, -(s - h)))]
    meshes = [Mesh(v, i, rr.LAMBERTIAN, base_color=(0.7, 0.7, 0.7, 1.0)) for v, i in parts]
    cam = rr.camera.Camera((-2.5, 0.6, 1.2), (-0.6, 2.5, -0.3), 60.0, width / height, 0.01, 1000.0)
    return Scene("fog_slab", [(Model(meshes, []), None)], [], cam)


def slab_view(scene, width=W, height=H, **kw):
    from hybrid_util import frame_view

    v = frame_view(scene, width, height, **kw)
    v.sun_dir[:] = SLAB_SUN
    return v


def slab_predicate(X, sun):
    """float64: (lit, compared, inside) of the sample points X (..., 3) of the slab scene under the direction `sun` toward the sun. Lit: the
    point lies above the sheet, or its projection along the sun direction onto the sheet's plane lands inside the hole. Compared: not
    within BOUNDARY of the sheet or of a shadow boundary (the planes the hole's four edges sweep along the sun direction). Inside: the
    projection of a point below the sheet lies a unit or more inside the sheet's span - what the predicate takes for granted"""
    X, s = np.asarray(X, np.float64), np.asarray(sun, np.float64)
    s = s / np.linalg.norm(s)
    above = X[..., 1] > SLAB_Y
    t = (SLAB_Y - X[..., 1]) / s[1]
    qx, qz = X[..., 0] + t * s[0], X[..., 2] + t * s[2]
    lit = above | ((np.abs(qx) < HOLE_HALF) & (np.abs(qz) < HOLE_HALF))
    # the perpendicular distance to the plane swept by the edge x = +-h (z = +-h): the in-plane distance times s_y / |(s_x, s_y)|
    dist_x = np.abs(np.abs(qx) - HOLE_HALF) * s[1] / np.hypot(s[0], s[1])
    dist_z = np.abs(np.abs(qz) - HOLE_HALF) * s[1] / np.hypot(s[2], s[1])
    margin = HOLE_HALF + 4 * BOUNDARY
    near_edge = ((dist_x < BOUNDARY) & (np.abs(qz) < margin)) | ((dist_z < BOUNDARY) & (np.abs(qx) < margin))
    compared = ~((np.abs(X[..., 1] - SLAB_Y) < BOUNDARY) | (~above & near_edge))
    inside_span = above | ((np.abs(qx) < SLAB_HALF - 1.0) & (np.abs(qz) < SLAB_HALF - 1.0))
    return lit, compared, inside_span

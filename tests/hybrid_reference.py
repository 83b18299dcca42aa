"""CPU reference of the hybrid graph's ray-traced passes (uh_render_hybrid): the G-buffer of gbuffer.vert / gbuffer.frag as a primary-ray
cast, rt_shadows and rt_reflections (IBL off). Composed from the oracle's primitives - primary_ray, trace_closest, offset_ray, sky,
sample_texture - plus numpy float32 in the order DESIGN.md section 2 "Hybrid passes" pins. Not a conftest: test modules import it."""
import numpy as np

import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.types import VERTEX_DTYPE

F = np.float32
MISS = 0xFFFFFFFF


def upload_recorded(scene, renderer, defaults=True):
    """scene.upload(renderer) with Renderer.initialize's four default maps first (so every material carries a normal, occlusion and
    metallic-roughness map), recording what each add_mesh call received: the references need the meshes as the shaders read them (the
    metallic / roughness factors: the deferred pass)"""
    meshes = []
    add = renderer.add_mesh

    def add_mesh(vertices, indices, material, world3x4=None):
        w = rr.identity3x4() if world3x4 is None else np.ascontiguousarray(world3x4, dtype=np.float32).reshape(12)
        meshes.append(dict(vertices=np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE), indices=np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1),
                           world=w.copy(), diffuse_map=material.diffuse_map, normal_map=material.normal_map,
                           metallic_roughness_map=material.metallic_roughness_map, occlusion_map=material.occlusion_map,
                           base_color=np.array(material.base_color_factor[:3], dtype=np.float32), type=float(material.raytrace_properties[0]),
                           metallic=F(material.metallic_factor), roughness=F(material.roughness_factor)))
        return add(vertices, indices, material, world3x4)

    renderer.add_mesh = add_mesh
    try:
        if defaults:
            renderer.initialize()
        scene.upload(renderer)
    finally:
        del renderer.add_mesh
    return meshes


# ---- the pinned arithmetic, vectorised over (N, 3) float32 arrays -------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(dot(a, a))
        return a * inv[..., None]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def mat3_mul(m, a):
    """mat3(world) * a, m row-major 3x3: ((col0 * x + col1 * y) + col2 * z)"""
    return np.stack([(m[3 * r] * a[..., 0] + m[3 * r + 1] * a[..., 1]) + m[3 * r + 2] * a[..., 2] for r in range(3)], axis=-1)


def inverse_transpose_mul(w2o, n):
    return np.stack([(n[..., 0] * w2o[i] + n[..., 1] * w2o[3 + i]) + n[..., 2] * w2o[6 + i] for i in range(3)], axis=-1)


def invert3x3(w):
    """the library's inverse of the upper 3x3 of a row-major 3x4 (scene_build.hip invert3x3: cofactor * (1 / det)); identity verbatim"""
    w = np.asarray(w, dtype=np.float32)
    if np.array_equal(w, rr.identity3x4()):
        return np.eye(3, dtype=np.float32).reshape(9)
    a, b, c, d, e, f, g, h, i = (w[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    A, B, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = (a * A + b * B) + c * C
    inv = F(1.0) / det
    return np.array([A * inv, -(b * i - c * h) * inv, (b * f - c * e) * inv, B * inv, (a * i - c * g) * inv, -(a * f - c * d) * inv,
                     C * inv, -(a * h - b * g) * inv, (a * e - b * d) * inv], dtype=np.float32)


def offset_ray(p, n):
    """view.glsl:92-108 offsetRay, vectorised: bit for bit oracle_api.offset_ray"""
    p, n = np.asarray(p, dtype=np.float32), np.asarray(n, dtype=np.float32)
    of = (F(256.0) * n).astype(np.int32)
    add = np.where(p < 0, -of, of).astype(np.uint32)
    with np.errstate(over="ignore"):
        pi = (p.view(np.uint32) + add).view(np.float32)
    return np.where(np.abs(p) < F(1.0 / 32.0), p + F(1.0 / 65536.0) * n, pi)


def unorm8(x):
    x = np.where(x > 0, x, F(0.0))
    x = np.where(x > 1, F(1.0), x)
    return np.rint(x * F(255.0)).astype(np.uint8)


def corner(img):
    """texture(image, vec2(px) / size) through LINEAR + MIRRORED_REPEAT: the mean of the 2x2 texels up and to the left"""
    H, W = img.shape[:2]
    y0, x0 = np.maximum(np.arange(H) - 1, 0), np.maximum(np.arange(W) - 1, 0)
    a, b, c, d = img[y0][:, x0], img[y0], img[:, x0], img
    return ((a + b) + (c + d)) * F(0.25)


def sun_direction(view):
    s = np.array(view.sun_dir[:], dtype=np.float32)
    return s * (F(1.0) / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))


def trace(oracle, origins, dirs):
    """closest hits through the oracle, tmin 0.001, tmax 10000: (t, u, v, mesh, prim)"""
    n = len(origins)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origins, 0.001, dirs, 10000.0
    tuv, mesh, prim = oracle.trace_closest(rays) if n else (np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    return tuv[:, 0], tuv[:, 1], tuv[:, 2], mesh, prim


def sample(oracle, tex, u, v):
    out = np.empty((len(u), 3), dtype=np.float32)
    for k in range(len(u)):
        out[k] = oracle.sample_texture(int(tex[k]), float(u[k]), float(v[k]))
    return out


def _uv(meshes, mesh, prim, b0, b1, b2):
    uu, vv = np.zeros(len(mesh), np.float32), np.zeros(len(mesh), np.float32)
    for m in np.unique(mesh):
        sel = mesh == m
        M = meshes[int(m)]
        tri = M["indices"].reshape(-1, 3)[prim[sel]]
        uv = [M["vertices"]["uv"][tri[:, k]] for k in range(3)]
        uu[sel] = (uv[0][:, 0] * b0[sel] + uv[1][:, 0] * b1[sel]) + uv[2][:, 0] * b2[sel]
        vv[sel] = (uv[0][:, 1] * b0[sel] + uv[1][:, 1] * b1[sel]) + uv[2][:, 1] * b2[sel]
    return uu, vv


def gbuffer(oracle, meshes, view, W, H):
    """the four targets of the hybrid G-buffer pass: dict(position, normal (H, W, 4) float32, albedo (H, W, 4) uint8, pbr (H, W, 4) float32)"""
    n = W * H
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    for pix in range(n):
        r = oa.primary_ray(view, W, H, pix % W, pix // W, 0.5, 0.5)
        o[pix], d[pix] = r[:3], r[3:]
    t, u, v, mesh, prim = trace(oracle, o, d)
    pos = np.tile(np.array([1, 1, 1, 0], np.float32), (n, 1))
    nrm, pbr = pos.copy(), pos.copy()
    alb = np.tile(np.array([255, 255, 255, 0], np.uint8), (n, 1))
    hit = mesh != MISS
    hi = np.nonzero(hit)[0]
    pos[hi, :3], pos[hi, 3] = o[hi] + t[hi, None] * d[hi], 1.0
    mesh, prim, u, v = mesh[hi], prim[hi], u[hi], v[hi]
    b0, b1, b2 = (F(1.0) - u) - v, u, v
    uu, vv = _uv(meshes, mesh, prim, b0, b1, b2)
    nn = np.zeros((len(hi), 3), np.float32)
    for m in np.unique(mesh):
        sel = np.nonzero(mesh == m)[0]
        M = meshes[int(m)]
        o2w = M["world"].reshape(3, 4)[:, :3].reshape(9)
        w2o = invert3x3(M["world"])
        tri = M["indices"].reshape(-1, 3)[prim[sel]]
        nk = [M["vertices"]["normal"][tri[:, k], :3] for k in range(3)]
        tk = [M["vertices"]["tangent"][tri[:, k], :3] for k in range(3)]
        L = lambda a, b, c: (a * b0[sel, None] + b * b1[sel, None]) + c * b2[sel, None]
        tangent = L(*tk)
        mapped = np.any(tangent != 0, axis=1)
        nn[sel] = normalize(L(*[inverse_transpose_mul(w2o, x) for x in nk]))
        if mapped.any():
            T = L(*[normalize(mat3_mul(o2w, tk[k])) for k in range(3)])
            B = L(*[normalize(mat3_mul(o2w, cross(nk[k], tk[k]))) for k in range(3)])
            N = L(*[normalize(mat3_mul(o2w, nk[k])) for k in range(3)])
            s = sel[mapped]
            nm = sample(oracle, np.full(len(s), M["normal_map"]), uu[s], vv[s])
            x = normalize(nm * F(2.0) - F(1.0))
            nn[s] = normalize((T[mapped] * x[:, 0:1] + B[mapped] * x[:, 1:2]) + N[mapped] * x[:, 2:3])
    nrm[hi, :3], nrm[hi, 3] = nn, 1.0
    maps = lambda key: np.array([meshes[int(m)][key] for m in mesh], dtype=np.uint32)
    diffuse = sample(oracle, maps("diffuse_map"), uu, vv)
    alb[hi, :3], alb[hi, 3] = unorm8(diffuse), 255
    mr, oc = sample(oracle, maps("metallic_roughness_map"), uu, vv), sample(oracle, maps("occlusion_map"), uu, vv)
    pbr[hi] = np.stack([mr[:, 2], mr[:, 1], oc[:, 0], mesh.astype(np.float32)], axis=1)
    shape = lambda a: a.reshape(H, W, -1)
    return dict(position=shape(pos), normal=shape(nrm), albedo=shape(alb), pbr=shape(pbr))


def shadows(oracle, position, normal, view):
    """rt_shadows.rgen: (H, W) uint8, 0 where the sun ray from the G-buffer's texel corner hits something, 255 where it does not"""
    H, W = position.shape[:2]
    p, n = corner(position)[..., :3].reshape(-1, 3), corner(normal)[..., :3].reshape(-1, 3)
    o = offset_ray(p, n)
    sun = np.broadcast_to(sun_direction(view), o.shape)
    _, _, _, mesh, _ = trace(oracle, o, sun)
    return np.where(mesh != MISS, 0, 255).astype(np.uint8).reshape(H, W)


def reflections(oracle, meshes, position, normal, pbr, view, furnace=False):
    """rt_reflections (IBL off): (H, W, 4) uint8 and the per-pixel class (0 not metal, 1 hit, 2 miss)"""
    H, W = position.shape[:2]
    p, n = corner(position)[..., :3].reshape(-1, 3), corner(normal)[..., :3].reshape(-1, 3)
    material = corner(pbr)[..., 3].reshape(-1).astype(np.uint32)
    types = np.array([m["type"] for m in meshes] + [0.0], dtype=np.float32)
    metal = types[np.minimum(material, len(meshes))] == 1.0
    out = np.zeros((H * W, 4), np.uint8)
    kind = np.zeros(H * W, np.uint8)
    idx = np.nonzero(metal)[0]
    o = offset_ray(p[idx], n[idx])
    eye = np.array(view.eye_pos[:], dtype=np.float32)
    I = -normalize(eye[None, :] - o)
    d = I - n[idx] * (F(2.0) * dot(n[idx], I))[:, None]
    t, u, v, mesh, prim = trace(oracle, o, d)
    hit = mesh != MISS
    c = np.zeros((len(idx), 3), np.float32)
    if hit.any():
        b0, b1, b2 = (F(1.0) - u[hit]) - v[hit], u[hit], v[hit]
        uu, vv = _uv(meshes, mesh[hit], prim[hit], b0, b1, b2)
        tex = sample(oracle, np.array([meshes[int(m)]["diffuse_map"] for m in mesh[hit]], np.uint32), uu, vv)
        base = np.array([meshes[int(m)]["base_color"] for m in mesh[hit]], np.float32).reshape(-1, 3)
        c[hit] = F(0.1) * (tex * base)
    for k in np.nonzero(~hit)[0]:
        c[k] = 1.0 if furnace else np.minimum(oa.sky(o[k], d[k], view.sun_dir[:]), F(1.0))
    out[idx, :3] = unorm8(c)
    kind[idx] = np.where(hit, 1, 2)
    return out.reshape(H, W, 4), kind.reshape(H, W)

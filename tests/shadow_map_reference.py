"""CPU reference of the cascaded shadow maps (uh_shadow_cascades, UH_HYBRID_SHADOW_MAPS and the deferred pass's calculateShadow) in
numpy, in the order DESIGN.md section 2 "Shadow maps" pins: setup_shadow_pass in float32 and in float64, the depth-only rasteriser
(transform, guard-band clip, 8-bit snap, top-left coverage, depth from the integer barycentrics, min) and the PCF lookup. Not a
conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr

F = np.float32
GUARD = F(524288.0)
ONE_BITS = np.uint32(0x3F800000)


# ---- setup_shadow_pass ----------------------------------------------------------------------------------------------------------
def _mat_mul(a, b):
    """column-major 4x4 (16,) product: element (r, c) = ((a(r,0) b(0,c) + a(r,1) b(1,c)) + a(r,2) b(2,c)) + a(r,3) b(3,c)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    o = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            o[4 * c + r] = ((a[r] * b[4 * c] + a[4 + r] * b[4 * c + 1]) + a[8 + r] * b[4 * c + 2]) + a[12 + r] * b[4 * c + 3]
    return o


def _inverse(m):
    """the GLM / glam scalar cofactor inverse, float32; None when the determinant is 0"""
    m = np.asarray(m, F)
    e = lambda c, r: m[4 * c + r]
    m00, m01, m02, m03 = (e(0, r) for r in range(4))
    m10, m11, m12, m13 = (e(1, r) for r in range(4))
    m20, m21, m22, m23 = (e(2, r) for r in range(4))
    m30, m31, m32, m33 = (e(3, r) for r in range(4))
    c00, c02, c03 = m22 * m33 - m32 * m23, m12 * m33 - m32 * m13, m12 * m23 - m22 * m13
    c04, c06, c07 = m21 * m33 - m31 * m23, m11 * m33 - m31 * m13, m11 * m23 - m21 * m13
    c08, c10, c11 = m21 * m32 - m31 * m22, m11 * m32 - m31 * m12, m11 * m22 - m21 * m12
    c12, c14, c15 = m20 * m33 - m30 * m23, m10 * m33 - m30 * m13, m10 * m23 - m20 * m13
    c16, c18, c19 = m20 * m32 - m30 * m22, m10 * m32 - m30 * m12, m10 * m22 - m20 * m12
    c20, c22, c23 = m20 * m31 - m30 * m21, m10 * m31 - m30 * m11, m10 * m21 - m20 * m11
    f0, f1, f2 = [c00, c00, c02, c03], [c04, c04, c06, c07], [c08, c08, c10, c11]
    f3, f4, f5 = [c12, c12, c14, c15], [c16, c16, c18, c19], [c20, c20, c22, c23]
    v0, v1, v2, v3 = [m10, m00, m00, m00], [m11, m01, m01, m01], [m12, m02, m02, m02], [m13, m03, m03, m03]
    sa, sb = [F(1), F(-1), F(1), F(-1)], [F(-1), F(1), F(-1), F(1)]
    inv = np.zeros(16, F)
    for i in range(4):
        inv[i] = ((v1[i] * f0[i] - v2[i] * f1[i]) + v3[i] * f2[i]) * sa[i]
        inv[4 + i] = ((v0[i] * f0[i] - v2[i] * f3[i]) + v3[i] * f4[i]) * sb[i]
        inv[8 + i] = ((v0[i] * f1[i] - v1[i] * f3[i]) + v3[i] * f5[i]) * sa[i]
        inv[12 + i] = ((v0[i] * f2[i] - v1[i] * f4[i]) + v2[i] * f5[i]) * sb[i]
    det = ((m00 * inv[0] + m01 * inv[4]) + m02 * inv[8]) + m03 * inv[12]
    if det == 0 or not np.isfinite(det):
        return None
    return inv * (F(1.0) / det)


def _v(x, y, z):
    return np.array([x, y, z], F)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return _v(a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _normalize(a):
    return a * (F(1.0) / np.sqrt(_dot(a, a)))


CORNERS = [(-1, 1, 0), (1, 1, 0), (1, -1, 0), (-1, -1, 0), (-1, 1, 1), (1, 1, 1), (1, -1, 1), (-1, -1, 1)]


def cascades_f32(view, proj, z_near, z_far, sun):
    """uh_shadow_cascades' pinned float32 order: (vp (4, 16) column-major, splits (4,)), or None where it refuses"""
    with np.errstate(all="ignore"):
        near, far = F(z_near), F(z_far)
        clip_range = far - near
        min_z, max_z = near, near + clip_range
        rng, ratio = max_z - min_z, max_z / min_z
        splits = []
        for i in range(4):
            p = F(i + 1) / F(4.0)
            lg = min_z * F(np.power(np.float64(ratio), np.float64(p)))
            uniform = min_z + rng * p
            d = F(0.927) * (lg - uniform) + uniform
            splits.append((d - near) / clip_range)
        inv = _inverse(_mat_mul(proj, view))
        if inv is None:
            return None
        sun = np.asarray(sun, F)
        vps, depths, last = np.zeros((4, 16), F), np.zeros(4, F), F(0.0)
        for i in range(4):
            split = splits[i]
            cs = []
            for c in CORNERS:
                h = [((inv[r] * F(c[0]) + inv[4 + r] * F(c[1])) + inv[8 + r] * F(c[2])) + inv[12 + r] * F(1.0) for r in range(4)]
                cs.append(_v(h[0] / h[3], h[1] / h[3], h[2] / h[3]))
            for k in range(4):
                dist = cs[k + 4] - cs[k]
                cs[k + 4] = cs[k] + dist * split
                cs[k] = cs[k] + dist * last
            center = _v(0, 0, 0)
            for k in range(8):
                center = center + cs[k]
            center = center / F(8.0)
            radius = F(0.0)
            for k in range(8):
                d = cs[k] - center
                radius = max(radius, np.sqrt(_dot(d, d)))
            radius = np.ceil(radius * F(16.0)) / F(16.0)
            eye = center - sun * (-radius)
            f = _normalize(eye - center)
            s = _normalize(_cross(_v(0, 1, 0), f))
            u = _cross(f, s)
            lv = np.array([s[0], u[0], f[0], 0, s[1], u[1], f[1], 0, s[2], u[2], f[2], 0, -_dot(s, eye), -_dot(u, eye), -_dot(f, eye), 1], F)
            left, right, bottom, top = -radius, radius, -radius, radius
            zn, zf = -(radius - -radius), radius - -radius
            rw, rh, rz = F(1.0) / (right - left), F(1.0) / (top - bottom), F(1.0) / (zn - zf)
            ortho = np.array([rw + rw, 0, 0, 0, 0, rh + rh, 0, 0, 0, 0, rz, 0, -(left + right) * rw, -(top + bottom) * rh, rz * zn, 1], F)
            vps[i] = _mat_mul(ortho, lv)
            depths[i] = near + split * clip_range
            last = split
    return vps, depths


def cascades_f64(view, proj, z_near, z_far, sun):
    """shadow.rs in float64 with numpy's own inverse: (vp (4, 4, 4) row-major matrices, splits (4,))"""
    V = np.asarray(view, np.float64).reshape(4, 4).T
    P = np.asarray(proj, np.float64).reshape(4, 4).T
    near, far = float(z_near), float(z_far)
    rng, ratio = far - near, far / near
    splits = []
    for i in range(4):
        p = (i + 1) / 4.0
        d = 0.927 * (near * ratio ** p - (near + rng * p)) + (near + rng * p)
        splits.append((d - near) / rng)
    inv = np.linalg.inv(P @ V)
    sun = np.asarray(sun, np.float64)
    vps, depths, last = [], [], 0.0
    for i in range(4):
        cs = [inv @ np.array([*c, 1.0]) for c in CORNERS]
        cs = [c[:3] / c[3] for c in cs]
        for k in range(4):
            dist = cs[k + 4] - cs[k]
            cs[k + 4] = cs[k] + dist * splits[i]
            cs[k] = cs[k] + dist * last
        center = sum(cs) / 8.0
        radius = max(np.linalg.norm(c - center) for c in cs)
        radius = np.ceil(radius * 16.0) / 16.0
        eye = center + sun * radius
        f = (eye - center) / np.linalg.norm(eye - center)
        s = np.cross([0.0, 1.0, 0.0], f)
        s /= np.linalg.norm(s)
        u = np.cross(f, s)
        lv = np.eye(4)
        lv[0, :3], lv[1, :3], lv[2, :3] = s, u, f
        lv[:3, 3] = [-s @ eye, -u @ eye, -f @ eye]
        ortho = np.eye(4)
        ortho[0, 0] = ortho[1, 1] = 1.0 / radius
        ortho[2, 2] = 1.0 / (-4.0 * radius)
        ortho[2, 3] = -2.0 * radius / (-4.0 * radius)
        vps.append(ortho @ lv)
        depths.append(near + splits[i] * rng)
        last = splits[i]
    return np.array(vps), np.array(depths)


def params_arrays(params):
    """(vp (4, 16), splits (4,)) float32 of a ShadowmapParams"""
    vp = np.array([list(params.view_projection_matrices[c]) for c in range(4)], F)
    return vp, np.array(params.cascade_splits[:], F)


# ---- the rasteriser -------------------------------------------------------------------------------------------------------------
def mesh_matrix(vp, world3x4):
    """vp (16,) times the instance's 3x4 with row (0, 0, 0, 1), column-major (16,)"""
    o = np.asarray(world3x4, F).reshape(3, 4)
    w = np.zeros(16, F)
    for c in range(4):
        for r in range(3):
            w[4 * c + r] = o[r, c]
        w[4 * c + 3] = F(1.0) if c == 3 else F(0.0)
    return _mat_mul(vp, w)


def _finish(a, b, c, S):
    """one screen-space triangle inside the guard band: a record (X (3,), Y (3,), z (3,), box) or None"""
    zs = np.array([a[2], b[2], c[2]], F)
    if (zs < 0).all() or (zs > 1).all():
        return None
    X = np.rint(np.array([a[0], b[0], c[0]], F) * F(256.0)).astype(np.int64)
    Y = np.rint(np.array([a[1], b[1], c[1]], F) * F(256.0)).astype(np.int64)
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return None
    if area < 0:
        X[[1, 2]], Y[[1, 2]], zs[[1, 2]] = X[[2, 1]], Y[[2, 1]], zs[[2, 1]]
    x0, x1 = max(-((-(X.min() - 128)) >> 8), 0), min((X.max() - 128) >> 8, S - 1)
    y0, y1 = max(-((-(Y.min() - 128)) >> 8), 0), min((Y.max() - 128) >> 8, S - 1)
    if x0 > x1 or y0 > y1:
        return None
    return X, Y, zs, (int(x0), int(x1), int(y0), int(y1))


def _clip(poly):
    """Sutherland-Hodgman against the guard band, DESIGN.md's order and intersection rule"""
    for p in range(4):
        axis, B = p >> 1, (GUARD if p & 1 else -GUARD)
        inside = (lambda q: q[axis] <= B) if p & 1 else (lambda q: q[axis] >= B)
        out = []
        n = len(poly)
        for i in range(n):
            cur, nxt = poly[i], poly[(i + 1) % n]
            ci, ni = inside(cur), inside(nxt)
            if ci:
                out.append(cur)
            if ci != ni:
                a, b = (cur, nxt) if ci else (nxt, cur)
                t = (B - a[axis]) / (b[axis] - a[axis])
                r = np.zeros(3, F)
                r[axis] = B
                o = 1 - axis
                r[o] = a[o] + t * (b[o] - a[o])
                r[2] = a[2] + t * (b[2] - a[2])
                out.append(r)
        poly = out
        if len(poly) < 3:
            return []
    for q in poly:
        if not (abs(q[0]) <= GUARD and abs(q[1]) <= GUARD and q[2] == q[2]):
            return []
    return poly


def records_for(meshes, vp, S):
    """the records (X, Y, z, box) of one cascade for meshes (hybrid_reference.upload_recorded's dicts)"""
    recs = []
    half = F(S) * F(0.5)
    nhalf = -half
    for m in meshes:
        M = mesh_matrix(vp, m["world"])
        p = m["vertices"]["pos"][:, :3].astype(F)
        with np.errstate(all="ignore"):
            xd = ((M[0] * p[:, 0] + M[4] * p[:, 1]) + M[8] * p[:, 2]) + M[12] * F(1.0)
            yd = ((M[1] * p[:, 0] + M[5] * p[:, 1]) + M[9] * p[:, 2]) + M[13] * F(1.0)
            zd = ((M[2] * p[:, 0] + M[6] * p[:, 1]) + M[10] * p[:, 2]) + M[14] * F(1.0)
            v = np.stack([xd * half + half, yd * nhalf + half, zd], axis=-1).astype(F)
        tri = v[m["indices"].reshape(-1, 3)]  # (T, 3, 3)
        finite = np.isfinite(tri).all(axis=(1, 2))
        z = tri[..., 2]
        x, y = tri[..., 0], tri[..., 1]
        keep = finite & ~(z < 0).all(1) & ~(z > 1).all(1) & ~(x < 0).all(1) & ~(y < 0).all(1) & ~(x > F(S)).all(1) & ~(y > F(S)).all(1)
        guard = ~((np.abs(x) <= GUARD) & (np.abs(y) <= GUARD)).all(1)
        for t in np.nonzero(keep)[0]:
            a, b, c = tri[t]
            if not guard[t]:
                r = _finish(a, b, c, S)
                if r is not None:
                    recs.append(r)
                continue
            poly = _clip([a.copy(), b.copy(), c.copy()])
            for j in range(1, len(poly) - 1):
                r = _finish(poly[0], poly[j], poly[j + 1], S)
                if r is not None:
                    recs.append(r)
    return recs


def _top_left(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _raster(rec, px, py):
    """(covered, z) at texel centres (px, py) (int64 arrays)"""
    X, Y, z, _ = rec
    Px, Py = px * 256 + 128, py * 256 + 128
    e0 = (X[2] - X[1]) * (Py - Y[1]) - (Y[2] - Y[1]) * (Px - X[1])
    e1 = (X[0] - X[2]) * (Py - Y[2]) - (Y[0] - Y[2]) * (Px - X[2])
    e2 = (X[1] - X[0]) * (Py - Y[0]) - (Y[1] - Y[0]) * (Px - X[0])
    cov = ((e0 > 0) | ((e0 == 0) & _top_left(X[2] - X[1], Y[2] - Y[1]))) & ((e1 > 0) | ((e1 == 0) & _top_left(X[0] - X[2], Y[0] - Y[2]))) & \
          ((e2 > 0) | ((e2 == 0) & _top_left(X[1] - X[0], Y[1] - Y[0])))
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    fa = F(area)
    with np.errstate(all="ignore"):
        l1, l2 = e1.astype(F) / fa, e2.astype(F) / fa
        zz = (z[0] + l1 * (z[1] - z[0])) + l2 * (z[2] - z[0])
    return cov & (zz >= 0) & (zz <= 1), zz


def rasterise(recs, S):
    """the D32 layer of these records: (S, S) float32, cleared to 1.0, min over fragments, -0 stored as +0"""
    depth = np.full(S * S, ONE_BITS, np.uint32)
    for rec in recs:
        x0, x1, y0, y1 = rec[3]
        py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        px, py = px.reshape(-1), py.reshape(-1)
        keep, zz = _raster(rec, px, py)
        if not keep.any():
            continue
        zz = np.where(zz == 0, F(0.0), zz).astype(F)
        np.minimum.at(depth, (py * S + px)[keep], zz[keep].view(np.uint32))
    return depth.view(F).reshape(S, S)


def shadow_maps(meshes, params, S):
    """all four layers (4, S, S) for the meshes and a ShadowmapParams"""
    vp, _ = params_arrays(params)
    return np.stack([rasterise(records_for(meshes, vp[c], S), S) for c in range(4)])


# ---- calculateShadow ------------------------------------------------------------------------------------------------------------
def _mirror(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _depth_tap(maps, c, S, x, y):
    ok = (np.abs(x) < F(1e9)) & (np.abs(y) < F(1e9))
    x, y = np.where(ok, x, F(0)), np.where(ok, y, F(0))
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = _mirror(ix, S), _mirror(ix + 1, S), _mirror(iy, S), _mirror(iy + 1, S)
    t = lambda yy, xx: maps[c, yy, xx]
    a = t(y0, x0) * (F(1.0) - ax) + t(y0, x1) * ax
    b = t(y1, x0) * (F(1.0) - ax) + t(y1, x1) * ax
    return np.where(ok, a * (F(1.0) - ay) + b * ay, F(0.0))


def calculate_shadow(P, view, params, maps):
    """shadow_mapping.glsl calculateShadow for (N, 3) float32 world positions: (factor (N,), cascade (N,))"""
    vp, splits = params_arrays(params)
    S = maps.shape[-1]
    V = np.array(view.view[:], F)
    with np.errstate(all="ignore"):
        vz = ((V[2] * P[:, 0] + V[6] * P[:, 1]) + V[10] * P[:, 2]) + V[14] * F(1.0)
        c = np.zeros(len(P), np.int64)
        for i in range(3):
            c = np.where(vz < -splits[i], i + 1, c)
        m = vp[c]  # (N, 16)
        row = lambda r: ((m[:, r] * P[:, 0] + m[:, 4 + r] * P[:, 1]) + m[:, 8 + r] * P[:, 2]) + m[:, 12 + r] * F(1.0)
        lx, ly, lz, lw = row(0), row(1), row(2), row(3)
        px, py, pz = lx / lw, ly / lw, lz / lw
        u, v = px * F(0.5) + F(0.5), F(1.0) - (py * F(0.5) + F(0.5))
        fS = F(S)
        ts = F(1.0) / fS
        inside = (pz <= F(1.0)) & (pz > F(-1.0))
        shadow = np.zeros(len(P), F)
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                uu, vv = u + F(x) * ts, v + F(y) * ts
                d = np.zeros(len(P), F)
                for k in range(4):
                    sel = inside & (c == k)
                    if sel.any():
                        d[sel] = _depth_tap(maps, k, S, (uu * fS - F(0.5))[sel], (vv * fS - F(0.5))[sel])
                tap = np.where((pz - F(0.0005)) > d, F(0.3), F(1.0))
                shadow = shadow + np.where(inside, tap, F(1.0))
        return (shadow / F(9.0)).astype(F), c


# ---- the deferred pass with shadows_enabled = 1 ---------------------------------------------------------------------------------------
def deferred_with_shadow_maps(g, reflections, ssao_img, view, meshes, params, maps, lights=()):
    """deferred.frag with shadows_enabled = 1 from hybrid_frame_reference.deferred: the rt_shadows branch neutralised (all 255
    multiplies by exactly 1.0) and SSAO off, then calculateShadow's factor and the SSAO factor in the reference's order. Returns the
    image (H, W, 4) and the cascade of every pixel (H, W)"""
    H, W = g["position"].shape[:2]
    v0 = type(view).from_buffer_copy(view)
    v0.ssao_enabled = 0
    ones = np.full((H, W), 255, np.uint8)
    base = fr.deferred(g, ones, reflections, None, v0, meshes, list(lights)).reshape(-1, 4)
    factor, cascade = calculate_shadow(g["position"][..., :3].reshape(-1, 3).astype(np.float32), view, params, maps)
    color = base[:, :3] * factor[:, None]
    if view.ssao_enabled == 1:
        color = color * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
    out = base.copy()
    out[:, :3] = color
    return out.reshape(H, W, 4), cascade.reshape(H, W)

"""CPU reference of the forward graph (uh_render_forward) in numpy, in the order DESIGN.md section 2 "Forward pass" pins: forward.vert's
clip position, the homogeneous clip to 0 <= z <= w, the divide and viewport, the shadow maps' guard-band clip, snap and top-left rule,
the depth test as the min of depth_bits << 32 | ~record, perspective-correct barycentrics and forward.frag. Not a conftest: test
modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_reference as hr
import shadow_map_reference as sr

F = np.float32
NONE = 0xFFFFFFFF
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def upload_recorded(scene, renderer, defaults=True):
    """hybrid_reference.upload_recorded, also recording the textures in the order added: (meshes, textures)"""
    textures = []
    add = renderer.add_texture

    def add_texture(rgba):
        textures.append(np.ascontiguousarray(rgba, dtype=np.uint8).copy())
        return add(rgba)

    renderer.add_texture = add_texture
    try:
        meshes = hr.upload_recorded(scene, renderer, defaults)
    finally:
        del renderer.add_texture
    return meshes, textures


def sample_texture(textures, index, u, v):
    """sample_texture (texture.rs: RGBA8 UNORM, LINEAR, MIRRORED_REPEAT, level 0) for (N,) texture indices and uv: (N, 3) float32"""
    index, u, v = np.asarray(index), np.asarray(u, F), np.asarray(v, F)
    out = np.ones((len(u), 3), F)
    for t in np.unique(index):
        sel = index == t
        if t >= len(textures):
            continue
        img = textures[int(t)]
        h, w = img.shape[:2]
        with np.errstate(all="ignore"):
            x, y = u[sel] * F(w) - F(0.5), v[sel] * F(h) - F(0.5)
            ok = (np.abs(x) < F(1e9)) & (np.abs(y) < F(1e9))
            x, y = np.where(ok, x, F(0)), np.where(ok, y, F(0))
            fx, fy = np.floor(x), np.floor(y)
            ax, ay = (x - fx)[:, None], (y - fy)[:, None]
            ix, iy = fx.astype(np.int64), fy.astype(np.int64)
            x0, x1, y0, y1 = sr._mirror(ix, w), sr._mirror(ix + 1, w), sr._mirror(iy, h), sr._mirror(iy + 1, h)
            tx = lambda yy, xx: fr.unorm_lut(img[yy, xx, :3])
            a = tx(y0, x0) * (F(1.0) - ax) + tx(y0, x1) * ax
            b = tx(y1, x0) * (F(1.0) - ax) + tx(y1, x1) * ax
            out[sel] = np.where(ok[:, None], a * (F(1.0) - ay) + b * ay, F(0.0))
    return out


# ---- the rasteriser -------------------------------------------------------------------------------------------------------------
def mesh_matrices(view, meshes):
    """(P V) W per mesh, column-major (16,): P V first, then the instance's 3x4 with row (0, 0, 0, 1)"""
    pv = sr._mat_mul(np.array(view.projection[:], F), np.array(view.view[:], F))
    return [sr.mesh_matrix(pv, m["world"]) for m in meshes]


def _clip_depth(poly):
    """Sutherland-Hodgman against z >= 0, then z <= w, on (x, y, z, w, b0, b1, b2) rows; crossings from the inside end"""
    for p in range(2):
        dist = (lambda q: q[3] - q[2]) if p else (lambda q: q[2])
        out = []
        n = len(poly)
        for i in range(n):
            cur, nxt = poly[i], poly[(i + 1) % n]
            dc, dn = dist(cur), dist(nxt)
            ci, ni = dc >= 0, dn >= 0
            if ci:
                out.append(cur)
            if ci != ni:
                a, b, da, db = (cur, nxt, dc, dn) if ci else (nxt, cur, dn, dc)
                t = da / (da - db)
                out.append((a + t * (b - a)).astype(F))
        poly = out
        if len(poly) < 3:
            return []
    return poly


def _guard_lerp(a, b, t, axis, B):
    """a guard-band crossing of screen vertices (x, y, z, w, b0, b1, b2): 1/w and b/w affine in screen space"""
    r = np.zeros(7, F)
    r[axis] = B
    o = 1 - axis
    r[o] = a[o] + t * (b[o] - a[o])
    r[2] = a[2] + t * (b[2] - a[2])
    ia, ib = F(1.0) / a[3], F(1.0) / b[3]
    iw = ia + t * (ib - ia)
    r[3] = F(1.0) / iw
    for j in range(3):
        pa, pb = a[4 + j] * ia, b[4 + j] * ib
        r[4 + j] = (pa + t * (pb - pa)) / iw
    return r


def _clip_guard(poly):
    for p in range(4):
        axis, B = p >> 1, (sr.GUARD if p & 1 else -sr.GUARD)
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
                out.append(_guard_lerp(a, b, t, axis, B))
        poly = out
        if len(poly) < 3:
            return []
    for q in poly:
        if not (abs(q[0]) <= sr.GUARD and abs(q[1]) <= sr.GUARD and q[2] == q[2]):
            return []
    return poly


def _finish(a, b, c, W, H, draw):
    zs = np.array([a[2], b[2], c[2]], F)
    if (zs < 0).all() or (zs > 1).all():
        return None
    X = np.rint(np.array([a[0], b[0], c[0]], F) * F(256.0)).astype(np.int64)
    Y = np.rint(np.array([a[1], b[1], c[1]], F) * F(256.0)).astype(np.int64)
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return None
    vs = [a, b, c]
    if area < 0:
        X[[1, 2]], Y[[1, 2]], zs[[1, 2]] = X[[2, 1]], Y[[2, 1]], zs[[2, 1]]
        vs = [a, c, b]
    x0, x1 = max(-((-(X.min() - 128)) >> 8), 0), min((X.max() - 128) >> 8, W - 1)
    y0, y1 = max(-((-(Y.min() - 128)) >> 8), 0), min((Y.max() - 128) >> 8, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    return dict(X=X, Y=Y, z=zs, box=(int(x0), int(x1), int(y0), int(y1)), w=np.array([q[3] for q in vs], F),
                B=np.array([q[4:7] for q in vs], F), draw=draw)


def _screen_triangle(a, b, c, W, H, draw):
    tri = np.stack([a, b, c])
    if not np.isfinite(tri[:, :3]).all():
        return []
    x, y, z = tri[:, 0], tri[:, 1], tri[:, 2]
    if (z < 0).all() or (z > 1).all() or (x < 0).all() or (y < 0).all() or (x > F(W)).all() or (y > F(H)).all():
        return []
    if ((np.abs(x) <= sr.GUARD) & (np.abs(y) <= sr.GUARD)).all():
        r = _finish(a, b, c, W, H, draw)
        return [r] if r is not None else []
    poly = _clip_guard([a.copy(), b.copy(), c.copy()])
    out = []
    for j in range(1, len(poly) - 1):
        r = _finish(poly[0], poly[j], poly[j + 1], W, H, draw)
        if r is not None:
            out.append(r)
    return out


def records_for(meshes, view, W, H):
    """every piece that reaches the rasteriser, in draw order: dicts of X, Y (int64), z, w (3,), B (3, 3) (rows: the piece's
    vertices after the winding swap), box and the draw index"""
    recs, draw = [], 0
    hw, hh = F(W) * F(0.5), F(H) * F(0.5)
    nhh = -hh
    for M, m in zip(mesh_matrices(view, meshes), meshes):
        p = m["vertices"]["pos"][:, :3].astype(F)
        with np.errstate(all="ignore"):
            clip = np.stack([((M[r] * p[:, 0] + M[4 + r] * p[:, 1]) + M[8 + r] * p[:, 2]) + M[12 + r] * F(1.0) for r in range(4)], axis=-1).astype(F)
        for tri in m["indices"].reshape(-1, 3):
            v = clip[tri]
            if not np.isfinite(v).all():
                draw += 1
                continue
            poly = [np.concatenate([v[k], np.eye(3, dtype=F)[k]]).astype(F) for k in range(3)]
            with np.errstate(all="ignore"):
                poly = _clip_depth(poly)
                s = []
                for q in poly:
                    xn, yn, zn = q[0] / q[3], q[1] / q[3], q[2] / q[3]
                    s.append(np.array([xn * hw + hw, yn * nhh + hh, zn, q[3], q[4], q[5], q[6]], F))
                for j in range(1, len(s) - 1):
                    recs.extend(_screen_triangle(s[0], s[j], s[j + 1], W, H, draw))
            draw += 1
    return recs


def _edges(rec, px, py):
    X, Y = rec["X"], rec["Y"]
    Px, Py = px * 256 + 128, py * 256 + 128
    e0 = (X[2] - X[1]) * (Py - Y[1]) - (Y[2] - Y[1]) * (Px - X[1])
    e1 = (X[0] - X[2]) * (Py - Y[2]) - (Y[0] - Y[2]) * (Px - X[2])
    e2 = (X[1] - X[0]) * (Py - Y[0]) - (Y[1] - Y[0]) * (Px - X[0])
    tl = sr._top_left
    cov = ((e0 > 0) | ((e0 == 0) & tl(X[2] - X[1], Y[2] - Y[1]))) & ((e1 > 0) | ((e1 == 0) & tl(X[0] - X[2], Y[0] - Y[2]))) & \
          ((e2 > 0) | ((e2 == 0) & tl(X[1] - X[0], Y[1] - Y[0])))
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    return cov, e0, e1, e2, F(area)


def _fragments(rec):
    """(pixel x, pixel y, depth) of the fragments the record keeps"""
    x0, x1, y0, y1 = rec["box"]
    py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    cov, e0, e1, e2, fa = _edges(rec, px, py)
    z = rec["z"]
    with np.errstate(all="ignore"):
        l1, l2 = e1.astype(F) / fa, e2.astype(F) / fa
        zz = ((z[0] + l1 * (z[1] - z[0])) + l2 * (z[2] - z[0])).astype(F)
    keep = cov & (zz >= 0) & (zz <= 1)
    return px[keep], py[keep], zz[keep]


def coverage_counts(recs, W, H):
    """fragments per pixel before the depth test, (H, W) int"""
    n = np.zeros(W * H, np.int64)
    for rec in recs:
        px, py, _ = _fragments(rec)
        np.add.at(n, py * W + px, 1)
    return n.reshape(H, W)


def resolve(recs, W, H):
    """the depth test: (depth (H, W) float32, visibility (H, W) uint32 draw index, record (H, W) int64, -1 for none)"""
    key = np.full(W * H, EMPTY_KEY, np.uint64)
    for r, rec in enumerate(recs):
        px, py, zz = _fragments(rec)
        if not len(px):
            continue
        bits = np.where(zz == 0, F(0.0), zz).astype(F).view(np.uint32).astype(np.uint64)
        k = (bits << np.uint64(32)) | np.uint64((~np.uint32(r)) & np.uint32(0xFFFFFFFF))
        np.minimum.at(key, py * W + px, k)
    empty = key == EMPTY_KEY
    depth = np.where(empty, np.uint32(0x3F800000), (key >> np.uint64(32)).astype(np.uint32)).view(F)
    rec = np.where(empty, -1, (~(key & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64))
    draws = np.array([r["draw"] for r in recs] or [0], np.int64)
    vis = np.where(empty, NONE, draws[np.maximum(rec, 0)]).astype(np.uint32)
    return depth.reshape(H, W), vis.reshape(H, W), rec.reshape(H, W)


def barycentrics(recs, rec, W, H):
    """the original triangles' perspective-correct barycentrics at the pixels with a record: (pixels (N,), b (N, 3))"""
    pix = np.nonzero(rec.reshape(-1) >= 0)[0]
    r = rec.reshape(-1)[pix]
    b = np.zeros((len(pix), 3), F)
    for k in np.unique(r):
        sel = r == k
        q = recs[int(k)]
        px, py = (pix[sel] % W).astype(np.int64), (pix[sel] // W).astype(np.int64)
        _, e0, e1, e2, fa = _edges(q, px, py)
        with np.errstate(all="ignore"):
            l = [e.astype(F) / fa for e in (e0, e1, e2)]
            qq = [l[i] / q["w"][i] for i in range(3)]
            s = (qq[0] + qq[1]) + qq[2]
            for j in range(3):
                b[sel, j] = ((qq[0] * q["B"][0, j] + qq[1] * q["B"][1, j]) + qq[2] * q["B"][2, j]) / s
    return pix, b


def triangle_of(meshes):
    """(mesh, prim) of every draw index"""
    mesh = np.concatenate([np.full(len(m["indices"]) // 3, i, np.int64) for i, m in enumerate(meshes)] or [np.zeros(0, np.int64)])
    prim = np.concatenate([np.arange(len(m["indices"]) // 3) for m in meshes] or [np.zeros(0, np.int64)])
    return mesh, prim


# ---- forward.frag ---------------------------------------------------------------------------------------------------------------
def direct_lighting(P, N, V, base, metallic, roughness, view, lights):
    """surfaceShading summed over k_hybrid_light_prep's records (the sun, then view.num_lights lights): the deferred pass's loop"""
    n = len(P)
    om = F(1.0) - metallic
    F0 = np.full((n, 3), F(0.04), F) * om[:, None] + base * metallic[:, None]
    NdotV = np.maximum(hr.dot(N, V), F(0.0))
    a = roughness * roughness
    a2 = a * a
    a2m1 = a2 - F(1.0)
    r1 = roughness + F(1.0)
    k = (r1 * r1) / F(8.0)
    omk = F(1.0) - k
    ggxV = NdotV / (NdotV * omk + k)
    nv4 = F(4.0) * NdotV
    Lo = np.zeros((n, 3), F)
    for rec in fr.light_records(view, list(lights)[: view.num_lights]):
        if rec["mode"] == 0:
            L, att = np.broadcast_to(rec["dir"], (n, 3)), np.ones(n, F)
        elif rec["mode"] == 3:
            L, att = np.zeros((n, 3), F), np.ones(n, F)
        else:
            ptl = rec["pos"][None, :] - P
            d = np.sqrt(hr.dot(ptl, ptl))
            L = ptl * (F(1.0) / d)[:, None]
            at = rec["att"]
            den = (at[0] * F(1.0) + at[1] * d) + at[2] * (d * d)
            if rec["mode"] == 2:
                att = np.power(np.maximum(hr.dot(L, rec["dir"][None, :]), F(0.0)), rec["spot"]) / den
            else:
                att = F(1.0) / den
        Hv = hr.normalize(V + L)
        rad = rec["color"][None, :] * att[:, None]
        NdotH = np.maximum(hr.dot(N, Hv), F(0.0))
        dn = (NdotH * NdotH) * a2m1 + F(1.0)
        dn = (fr.PI * dn) * dn
        NDF = a2 / dn
        NdotL = np.maximum(hr.dot(N, L), F(0.0))
        G = (NdotL / (NdotL * omk + k)) * ggxV
        x = np.minimum(np.maximum(F(1.0) - np.maximum(hr.dot(Hv, V), F(0.0)), F(0.0)), F(1.0))
        p5 = ((x * x) * (x * x)) * x
        Fr = F0 + (F(1.0) - F0) * p5[:, None]
        kD = (F(1.0) - Fr) * om[:, None]
        NG = NDF * G
        den2 = nv4 * NdotL + F(0.0001)
        spec = (NG[:, None] * Fr) / den2[:, None]
        c = (kD * base) / fr.PI + spec
        Lo = Lo + (c * rad) * NdotL[:, None]
    return Lo


def surface(meshes, textures, recs, rec, W, H):
    """forward.vert's attributes at the surviving fragments: (pixels, mesh, world position, normal, uv)"""
    pix, b = barycentrics(recs, rec, W, H)
    draw = np.array([recs[int(k)]["draw"] for k in rec.reshape(-1)[pix]], np.int64)
    tmesh, tprim = triangle_of(meshes)
    mesh, prim = tmesh[draw], tprim[draw]
    P, nn = np.zeros((len(pix), 3), F), np.zeros((len(pix), 3), F)
    uu, vv = np.zeros(len(pix), F), np.zeros(len(pix), F)
    b0, b1, b2 = b[:, 0], b[:, 1], b[:, 2]
    with np.errstate(all="ignore"):
        for mi in np.unique(mesh):
            sel = np.nonzero(mesh == mi)[0]
            M = meshes[int(mi)]
            o = M["world"].reshape(12)
            o2w = M["world"].reshape(3, 4)[:, :3].reshape(9)
            w2o = hr.invert3x3(M["world"])
            tri = M["indices"].reshape(-1, 3)[prim[sel]]
            L = lambda a, bb, c: (a * b0[sel, None] + bb * b1[sel, None]) + c * b2[sel, None]
            pk = [M["vertices"]["pos"][tri[:, k], :3].astype(F) for k in range(3)]
            wk = [np.stack([((o[4 * r] * q[:, 0] + o[4 * r + 1] * q[:, 1]) + o[4 * r + 2] * q[:, 2]) + o[4 * r + 3] * F(1.0) for r in range(3)], -1) for q in pk]
            P[sel] = L(*wk)
            uv = [M["vertices"]["uv"][tri[:, k]] for k in range(3)]
            uu[sel] = (uv[0][:, 0] * b0[sel] + uv[1][:, 0] * b1[sel]) + uv[2][:, 0] * b2[sel]
            vv[sel] = (uv[0][:, 1] * b0[sel] + uv[1][:, 1] * b1[sel]) + uv[2][:, 1] * b2[sel]
            nk = [M["vertices"]["normal"][tri[:, k], :3] for k in range(3)]
            tk = [M["vertices"]["tangent"][tri[:, k], :3] for k in range(3)]
            mapped = np.any(L(*tk) != 0, axis=1)
            nn[sel] = hr.normalize(L(*[hr.inverse_transpose_mul(w2o, x) for x in nk]))
            if mapped.any():
                T = L(*[hr.normalize(hr.mat3_mul(o2w, tk[k])) for k in range(3)])
                B = L(*[hr.normalize(hr.mat3_mul(o2w, hr.cross(nk[k], tk[k]))) for k in range(3)])
                N = L(*[hr.normalize(hr.mat3_mul(o2w, nk[k])) for k in range(3)])
                s = sel[mapped]
                nm = sample_texture(textures, np.full(len(s), M["normal_map"]), uu[s], vv[s])
                x = hr.normalize(nm * F(2.0) - F(1.0))
                nn[s] = hr.normalize((T[mapped] * x[:, 0:1] + B[mapped] * x[:, 1:2]) + N[mapped] * x[:, 2:3])
    return pix, mesh, P, nn, uu, vv


def forward(meshes, textures, view, lights, W, H, shadow=None):
    """the forward pass: dict(output (H, W, 4), depth (H, W), visibility (H, W), position (N, 3) and pixels (N,) of the covered
    pixels, records); shadow = (params, maps) when view.shadows_enabled == 1"""
    recs = records_for(meshes, view, W, H)
    depth, vis, rec = resolve(recs, W, H)
    out = np.tile(np.array([1, 1, 1, 0], F), (W * H, 1))
    pix, mesh, P, N, uu, vv = surface(meshes, textures, recs, rec, W, H)
    if len(pix):
        maps = lambda key: np.array([meshes[int(m)][key] for m in mesh], np.uint32)
        with np.errstate(all="ignore"):
            dt = sample_texture(textures, maps("diffuse_map"), uu, vv)
            mr = sample_texture(textures, maps("metallic_roughness_map"), uu, vv)
            oc = sample_texture(textures, maps("occlusion_map"), uu, vv)
            diffuse = np.power(dt.astype(np.float64), np.float64(F(2.2))).astype(F)
            bc = np.array([meshes[int(m)]["base_color"] for m in mesh], F)
            base = diffuse * bc
            metallic, roughness, occlusion = mr[:, 2], mr[:, 1], oc[:, 0]
            eye = np.array(view.eye_pos[:], F)
            V = hr.normalize(eye[None, :] - P)
            Lo = direct_lighting(P, N, V, base, metallic, roughness, view, lights)
            color = (F(0.03) * diffuse) * occlusion[:, None] + Lo
            if view.shadows_enabled == 1:
                params, smaps = shadow
                color = color * sr.calculate_shadow(P, view, params, smaps)[0][:, None]
        out[pix, :3], out[pix, 3] = color, 1.0
    return dict(output=out.reshape(H, W, 4), depth=depth, visibility=vis, position=P, pixels=pix, records=recs)


def present(output, view):
    """the present pass on forward_output: (H, W, 4) uint8 B, G, R, A"""
    return fr.present(output, fxaa_enabled=view.fxaa_enabled == 1)

"""CPU reference of the hybrid graph's rasterised G-buffer (uh_render_hybrid with UH_HYBRID_GBUFFER | UH_HYBRID_GBUFFER_RASTER) in numpy,
in the order DESIGN.md section 2 "Rasterised G-buffer" pins: the forward pass's rasteriser and fragment prologue (forward_reference),
then gbuffer.frag's four targets as the cast writes them (hybrid_reference.gbuffer). Not a conftest: test modules import it."""
import numpy as np

import forward_reference as fw
import hybrid_reference as hr
import oracle_api as oa

F = np.float32
NONE = fw.NONE


def _subset(meshes, draws):
    """the meshes with only the triangles of the draw indices `draws` (sorted, unique) kept, and the original draw index of each kept
    triangle in the subset's draw order"""
    out, orig, first = [], [], 0
    for m in meshes:
        n = len(m["indices"]) // 3
        keep = draws[(draws >= first) & (draws < first + n)] - first
        sub = dict(m)
        sub["indices"] = m["indices"].reshape(-1, 3)[keep].reshape(-1)
        out.append(sub)
        orig.append(keep + first)
        first += n
    return out, np.concatenate(orig or [np.zeros(0, np.int64)]).astype(np.int64)


def gbuffer_raster(meshes, textures, view, W, H, draws=None):
    """the pass: dict(position, normal (H, W, 4) float32, albedo (H, W, 4) uint8, pbr (H, W, 4) float32, depth (H, W) float32,
    visibility (H, W) uint32 draw index, records). draws: restate only those triangles (a subset: the result holds where the subset's
    surviving fragment is the whole scene's, e.g. where the visibility equals the device's)"""
    orig = None
    if draws is not None:
        meshes, orig = _subset(meshes, np.unique(np.asarray(draws, np.int64)))
    recs = fw.records_for(meshes, view, W, H)
    depth, vis, rec = fw.resolve(recs, W, H)
    if orig is not None:
        vis = np.where(vis == NONE, NONE, orig[np.minimum(vis, max(len(orig) - 1, 0)).astype(np.int64)]).astype(np.uint32)
    n = W * H
    pos = np.tile(np.array([1, 1, 1, 0], F), (n, 1))
    nrm, pbr = pos.copy(), pos.copy()
    alb = np.tile(np.array([255, 255, 255, 0], np.uint8), (n, 1))
    pix, mesh, P, N, uu, vv = fw.surface(meshes, textures, recs, rec, W, H)
    if len(pix):
        maps = lambda key: np.array([meshes[int(m)][key] for m in mesh], np.uint32)
        with np.errstate(all="ignore"):
            dt = fw.sample_texture(textures, maps("diffuse_map"), uu, vv)
            mr = fw.sample_texture(textures, maps("metallic_roughness_map"), uu, vv)
            oc = fw.sample_texture(textures, maps("occlusion_map"), uu, vv)
        pos[pix, :3], pos[pix, 3] = P, 1.0
        nrm[pix, :3], nrm[pix, 3] = N, 1.0
        alb[pix, :3], alb[pix, 3] = hr.unorm8(dt), 255
        pbr[pix] = np.stack([mr[:, 2], mr[:, 1], oc[:, 0], mesh.astype(F)], axis=1)
    shape = lambda a: a.reshape(H, W, -1)
    return dict(position=shape(pos), normal=shape(nrm), albedo=shape(alb), pbr=shape(pbr), depth=depth, visibility=vis, records=recs)


def cast_hits(oracle, view, W, H):
    """the cast's primary hits (hybrid_reference.gbuffer's rays): (mesh (H, W), prim (H, W), position (H, W, 3)); mesh hr.MISS where
    the ray missed"""
    n = W * H
    o, d = np.empty((n, 3), F), np.empty((n, 3), F)
    for pix in range(n):
        r = oa.primary_ray(view, W, H, pix % W, pix // W, 0.5, 0.5)
        o[pix], d[pix] = r[:3], r[3:]
    t, _, _, mesh, prim = hr.trace(oracle, o, d)
    p = o + t[:, None] * d
    return mesh.reshape(H, W), prim.reshape(H, W), p.reshape(H, W, 3)


def next_to_an_edge(a, b):
    """(H, W) bool: some pixel of the 3 x 3 neighbourhood differs from the centre in `a` or in `b` (two id images)"""
    H, W = a.shape
    edge = np.zeros((H, W), bool)
    for img in (a, b):
        pad = np.pad(img, 1, mode="edge")
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                edge |= pad[1 + dy : 1 + dy + H, 1 + dx : 1 + dx + W] != img
    return edge

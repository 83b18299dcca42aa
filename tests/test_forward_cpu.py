"""CPU: the forward graph's C ABI (uh_render_forward, uh_read_forward, uh_get_forward_stats), its Python and C++ surfaces, the oracle's
refusal, and known answers of the numpy restatement the GPU pass is held to bit for bit (tests/forward_reference.py): watertight
coverage, the near-plane clip, the depth test's tie rule, degenerate input and perspective-correct interpolation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import forward_reference as fw
import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.scenes import quad
from rust_renderer_amd.types import VERTEX_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
VERBS = ("uh_render_forward", "uh_read_forward", "uh_get_forward_stats")
F = np.float32


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_verbs_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in VERBS:
        assert re.search(r"\bint " + n + r"\(uh_ctx\* ctx", text), n
        assert "uh_mgpu_" + n[3:] not in text, "per-context only"
    lib = rr.load_library()
    for n in VERBS:
        assert hasattr(lib, n), n


def test_header_enums_and_layout_match_python(tmp_path):
    src = tmp_path / "l.c"
    names = ["UH_FORWARD_PASS", "UH_FORWARD_PRESENT", "UH_FORWARD_SHADOW_MAPS", "UH_FORWARD_GRAPH", "UH_FORWARD_OUTPUT", "UH_FORWARD_DEPTH",
             "UH_FORWARD_VISIBILITY", "UH_FORWARD_PRESENT_OUTPUT"]
    fields = ["renders", "pieces", "covered_pixels", "lights"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void){\n'
                   + "".join(f'printf("%d\\n", (int){n});\n' for n in names)
                   + 'printf("%d\\n", (int)sizeof(UhForwardStats));\n'
                   + "".join(f'printf("%d\\n", (int)offsetof(UhForwardStats, {f}));\n' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-std=c89", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.split()]
    S = rr.types.ForwardStats
    want = [rr.FORWARD_PASS, rr.FORWARD_PRESENT, rr.FORWARD_SHADOW_MAPS, rr.FORWARD_GRAPH, rr.FORWARD_OUTPUT, rr.FORWARD_DEPTH,
            rr.FORWARD_VISIBILITY, rr.FORWARD_PRESENT_OUTPUT, C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want
    assert rr.FORWARD_SHADOW_MAPS == rr.HYBRID_SHADOW_MAPS and rr.FORWARD_GRAPH == rr.FORWARD_SHADOW_MAPS | 3


def test_oracle_renderer_refuses_the_forward_verbs():
    r = oa.OracleRenderer(8, 8)
    v = rr.default_view(rr.camera.Camera((0, 0, 3), (0, 0, 0)), 8, 8)
    for call in (lambda: r.render_forward(v), lambda: r.read_forward(rr.FORWARD_OUTPUT), lambda: r.forward_stats()):
        with pytest.raises(NotImplementedError, match="forward graph"):
            call()


def test_cpp_mirror_builds_and_links(tmp_path):
    lib_dir = os.path.dirname(rr.build_library())
    exe = tmp_path / "forward_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "forward_host.cpp"),
                    "-L", lib_dir, "-lutopian_hip", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    assert exe.exists()


def test_texture_sampler_matches_the_oracle():
    r = oa.OracleRenderer(8, 8)
    textures = []
    add = r.add_texture

    def add_texture(rgba):
        textures.append(np.ascontiguousarray(rgba, np.uint8).copy())
        return add(rgba)

    r.add_texture = add_texture
    rng = np.random.default_rng(3)
    for w, h in ((7, 5), (32, 32), (1, 1)):
        r.add_texture(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))
    n = 400
    idx = rng.integers(0, len(textures), n)
    u, v = rng.uniform(-2.5, 3.5, n).astype(F), rng.uniform(-2.5, 3.5, n).astype(F)
    got = fw.sample_texture(textures, idx, u, v)
    want = np.array([r.sample_texture(int(idx[k]), float(u[k]), float(v[k])) for k in range(n)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (fw.sample_texture(textures, [len(textures)], [0.5], [0.5]) == 1.0).all(), "an index past the table reads white"


# ---- known answers of the restatement ---------------------------------------------------------------------------------------------
def _mesh(pos, indices, uv=None, world=None):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["pos"][:, :3], v["pos"][:, 3] = pos, 1.0
    if uv is not None:
        v["uv"] = uv
    return dict(vertices=v, indices=np.asarray(indices, np.uint32).reshape(-1), world=rr.identity3x4() if world is None else np.asarray(world, F))


def _view(eye, target, W, H, near=0.1, far=100.0, fov=60.0):
    return rr.default_view(rr.camera.Camera(eye, target, fov, W / H, near, far), W, H)


def _quad_mesh(origin, eu, ev, nu=1, nv=1):
    v, i = quad(origin, eu, ev, nu=nu, nv=nv)
    return dict(vertices=v, indices=np.asarray(i, np.uint32).reshape(-1), world=rr.identity3x4())


def _pixel_rays(view, W, H):
    """float64 rays through the pixel centres: (eye (3,), unit directions (H, W, 3)), NDC y = +1 at row 0"""
    P = np.array(view.projection[:], np.float64).reshape(4, 4).T
    V = np.array(view.view[:], np.float64).reshape(4, 4).T
    inv = np.linalg.inv(P @ V)
    x = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    y = 1.0 - (np.arange(H) + 0.5) / H * 2.0
    X, Y = np.meshgrid(x, y)
    def unproject(z):
        h = np.stack([X, Y, np.full_like(X, z), np.ones_like(X)], -1) @ inv.T
        return h[..., :3] / h[..., 3:]
    a, b = unproject(0.0), unproject(1.0)
    d = b - a
    return a, d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_split_quad_covers_every_centre_inside_exactly_once():
    W, H = 48, 40
    view = _view((0.3, 0.2, 3.0), (0.0, 0.0, 0.0), W, H)
    m = _quad_mesh((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
    recs = fw.records_for([m], view, W, H)
    assert len(recs) == 2
    n = fw.coverage_counts(recs, W, H)
    o, d = _pixel_rays(view, W, H)
    t = -o[..., 2] / d[..., 2]
    p = o + t[..., None] * d
    inside = (np.abs(p[..., 0]) < 0.97) & (np.abs(p[..., 1]) < 0.97)
    outside = (np.abs(p[..., 0]) > 1.03) | (np.abs(p[..., 1]) > 1.03)
    assert inside.sum() > 300
    assert (n[inside] == 1).all() and (n[outside] == 0).all() and n.max() == 1


def _cube():
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = []
    for a, b, cc, d in faces:
        idx += [a, b, cc, a, cc, d]
    return _mesh(c, idx)


def test_closed_cube_seen_from_outside_has_no_holes():
    W, H = 64, 48
    view = _view((2.6, 2.1, 3.4), (0.0, 0.0, 0.0), W, H)
    m = _cube()
    recs = fw.records_for([m], view, W, H)
    depth, vis, _ = fw.resolve(recs, W, H)
    o, d = _pixel_rays(view, W, H)
    # the ray through each centre hits the cube (slab test, float64) with a margin of 1% of the cube on every face
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-0.99 - o) / d, (0.99 - o) / d
    tmin, tmax = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    hit = tmin < tmax
    assert hit.sum() > 500
    assert (vis[hit] != fw.NONE).all(), "a pixel inside the silhouette was left uncovered"
    n = fw.coverage_counts(recs, W, H)
    assert (n[hit] == 2).all(), "front and back faces: each centre exactly once per side"


def test_floor_crossing_the_near_plane_is_clipped_and_watertight():
    W, H = 64, 48
    view = _view((0.0, 1.0, 0.0), (0.0, 0.2, -4.0), W, H, near=0.5, far=30.0)
    m = _quad_mesh((-20.0, 0.0, 20.0), (40.0, 0.0, 0.0), (0.0, 0.0, -40.0), nu=5, nv=5)
    recs = fw.records_for([m], view, W, H)
    depth, vis, _ = fw.resolve(recs, W, H)
    assert (depth >= 0).all() and (depth <= 1).all()
    assert all((r["z"] >= -1e-6).all() for r in recs)
    n = fw.coverage_counts(recs, W, H)
    o, d = _pixel_rays(view, W, H)
    t = -o[..., 1] / d[..., 1]
    p = o + t[..., None] * d
    fwd = np.array([0.0, -0.8, -4.0]) / np.linalg.norm([0.0, -0.8, -4.0])
    vz = (p - np.array([0.0, 1.0, 0.0])) @ fwd
    on = (t > 0) & (np.abs(p[..., 0]) < 19.5) & (np.abs(p[..., 2]) < 19.5) & (vz < 29.0)
    assert on.sum() > 800
    assert (n[on] == 1).all(), "every floor pixel exactly once across the clipped, shared edges"


def test_triangle_behind_the_eye_emits_nothing():
    W, H = 32, 32
    view = _view((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    m = _mesh([(-1.0, -1.0, 2.0), (1.0, -1.0, 2.0), (0.0, 1.0, 2.0)], [0, 1, 2])
    assert fw.records_for([m], view, W, H) == []


def test_coplanar_overlap_the_later_triangle_and_mesh_win():
    W, H = 32, 24
    view = _view((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), W, H)
    tri = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.0, 0.0)]
    a = _mesh(tri + tri, [0, 1, 2, 3, 5, 4])  # draw 1 with the other winding
    b = _mesh(tri, [0, 1, 2])
    _, vis, _ = fw.resolve(fw.records_for([a], view, W, H), W, H)
    assert set(np.unique(vis)) == {1, fw.NONE}
    _, vis, _ = fw.resolve(fw.records_for([a, b], view, W, H), W, H)
    assert set(np.unique(vis)) == {2, fw.NONE}, "mesh 1's triangle is draw 2"


def test_zero_area_and_nan_triangles_emit_nothing():
    W, H = 32, 32
    view = _view((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), W, H)
    line = _mesh([(-1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)], [0, 1, 2])
    point = _mesh([(0.2, 0.2, 0.0)] * 3, [0, 1, 2])
    nan = _mesh([(np.nan, 0.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.0, 0.0)], [0, 1, 2])
    for m in (line, point, nan):
        assert fw.records_for([m], view, W, H) == []


def test_uv_is_perspective_correct_on_a_steep_receding_plane():
    W, H = 128, 128
    view = _view((0.0, 1.5, 0.0), (0.0, 0.0, -3.0), W, H, near=0.1, far=50.0)
    L = 8.0  # w runs from 1.1 to 8.3 across it
    pos = [(-2.0, 0.0, -0.5), (2.0, 0.0, -0.5), (2.0, 0.0, -0.5 - L), (-2.0, 0.0, -0.5 - L)]
    uv = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    m = _mesh(pos, [0, 1, 2, 0, 2, 3], uv=uv)
    recs = fw.records_for([m], view, W, H)
    _, _, rec = fw.resolve(recs, W, H)
    pix, b = fw.barycentrics(recs, rec, W, H)
    assert len(pix) > 1500
    tri = m["indices"].reshape(-1, 3)
    draw = np.array([recs[int(k)]["draw"] for k in rec.reshape(-1)[pix]])
    uvs = np.array(uv, F)[tri[draw]]  # (N, 3, 2)
    got = (uvs[:, 0] * b[:, 0:1] + uvs[:, 1] * b[:, 1:2]) + uvs[:, 2] * b[:, 2:3]
    o, d = _pixel_rays(view, W, H)
    o, d = o.reshape(-1, 3)[pix], d.reshape(-1, 3)[pix]
    t = -o[:, 1] / d[:, 1]
    p = o + t[:, None] * d
    want = np.stack([(p[:, 0] + 2.0) / 4.0, (-0.5 - p[:, 2]) / L], -1)
    assert np.abs(got - want).max() < 1e-4
    # the affine (screen-space) weights of the same pieces miss by far more
    aff = np.zeros_like(b)
    for k in np.unique(rec.reshape(-1)[pix]):
        sel = rec.reshape(-1)[pix] == k
        q = recs[int(k)]
        _, e0, e1, e2, fa = fw._edges(q, (pix[sel] % W).astype(np.int64), (pix[sel] // W).astype(np.int64))
        l = np.stack([e.astype(F) / fa for e in (e0, e1, e2)], -1)
        aff[sel] = l @ q["B"]
    affine = (uvs[:, 0] * aff[:, 0:1] + uvs[:, 1] * aff[:, 1:2]) + uvs[:, 2] * aff[:, 2:3]
    assert np.abs(affine - want).max() > 1e-2

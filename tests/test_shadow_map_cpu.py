"""CPU: the cascaded shadow maps' C ABI (uh_shadow_cascades and the per-context verbs), setup_shadow_pass's host arithmetic against a
float64 reading of shadow.rs and against the float32 restatement of DESIGN.md's pinned order, its refusals, and known answers of the
numpy rasteriser that the GPU maps are held to (tests/shadow_map_reference.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rust_renderer_amd as rr
import shadow_map_reference as sr
from rust_renderer_amd import camera as cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "utopian_hip.h")
VERBS = ("uh_shadow_cascades", "uh_set_shadowmap_params", "uh_read_shadow_map", "uh_get_shadow_map_stats")
REF_SUN = tuple(np.float32(np.array([0.0, 0.9, 0.15]) / np.linalg.norm([0.0, 0.9, 0.15])))  # prototype/src/main.rs:69


def test_verbs_are_declared_after_the_group_section_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert text.index("uh_mgpu_set_option(") < min(text.index(n + "(") for n in VERBS)
    assert "uh_mgpu_shadow" not in text and "uh_mgpu_set_shadowmap" not in text
    lib = rr.load_library()
    for n in VERBS:
        assert hasattr(lib, n), n
    assert rr.HYBRID_SHADOW_MAPS == 256 and rr.HYBRID_FRAME == 0x7F


def test_struct_layouts_match_ctypes(tmp_path):
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "utopian_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   " sizeof(UhShadowmapParams), offsetof(UhShadowmapParams, cascade_splits), sizeof(UhShadowMapStats),"
                   " offsetof(UhShadowMapStats, triangles), offsetof(UhShadowMapStats, params), (int)UH_HYBRID_SHADOW_MAPS); return 0;}\n")
    subprocess.run(["gcc", "-std=c89", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.split()]
    T = rr.types
    assert got == [C.sizeof(T.ShadowmapParams), T.ShadowmapParams.cascade_splits.offset, C.sizeof(T.ShadowMapStats),
                   T.ShadowMapStats.triangles.offset, T.ShadowMapStats.params.offset, rr.HYBRID_SHADOW_MAPS] == [272, 256, 304, 12, 32, 256]


def _cameras():
    rng = np.random.default_rng(7)
    # the reference's view: prototype/src/main.rs:44-51 places the camera at (0, 2, 0) aiming at (0, 0.5, 0), straight down, where
    # camera.rs get_lookat_rotation's cross(forward, +Y) fails to normalise and the rotation falls back to identity: the camera looks
    # along -Z from (0, 2, 0). (Straight down itself would make look_at_rh singular.)
    out = [(cam.Camera((0.0, 2.0, 0.0), (0.0, 2.0, -1.0), 60.0, 1920 / 1080, 0.01, 1000.0), REF_SUN)]
    for _ in range(24):
        pos = rng.uniform(-20, 20, 3)
        tgt = pos + rng.normal(size=3)
        near = float(10 ** rng.uniform(-1.5, 0.5))
        far = near * float(10 ** rng.uniform(1, 3))
        sun = rng.normal(size=3)
        out.append((cam.Camera(pos, tgt, float(rng.uniform(30, 90)), float(rng.uniform(0.5, 2.5)), near, far), tuple(np.float32(sun))))
    return out


@pytest.mark.parametrize("k", range(25))
def test_cascades_match_float64_and_the_pinned_float32_order(k):
    c, sun = _cameras()[k]
    p = rr.shadow_cascades(c, sun)
    vp, splits = sr.params_arrays(p)
    V, P = cam.to_glam(c.get_view()), cam.to_glam(c.get_projection())
    f32 = sr.cascades_f32(V, P, c.z_near, c.z_far, sun)
    assert np.array_equal(f32[0].view(np.uint32), vp.view(np.uint32)) and np.array_equal(f32[1].view(np.uint32), splits.view(np.uint32))
    g, gs = sr.cascades_f64(V, P, c.z_near, c.z_far, np.asarray(sun, np.float64))
    assert np.allclose(splits, gs, rtol=2e-6, atol=0)
    # float32 itself (as the reference's glam): the inverse of projection * view has a condition number of about far / near, so its
    # far corners - and the cascades' centres and radii - carry a relative error of about far / near * 2^-24 (measured at most
    # 2.7e-7 * far / near over these cameras); 1e-5 plus eight units of that, and never more than 1e-3 (the reference's 0.01 / 1000)
    rtol = min(1e-5 + 8.0 * 2.0 ** -24 * (c.z_far / c.z_near), 1e-3)
    for i in range(4):
        ref = g[i].T.reshape(16)
        assert np.abs(vp[i] - ref).max() <= rtol * np.abs(ref).max(), (i, np.abs(vp[i] - ref).max() / np.abs(ref).max())
        assert np.array_equal(vp[i].reshape(4, 4)[:, 3], [0, 0, 0, 1])  # last row (0, 0, 0, 1): w = 1 in the rasteriser


def _call(view, proj, near, far, sun):
    lib = rr.load_library()
    fp = C.POINTER(C.c_float)
    lib.uh_shadow_cascades.argtypes = [fp, fp, C.c_float, C.c_float, fp, C.POINTER(rr.types.ShadowmapParams)]
    out = rr.types.ShadowmapParams()
    out.cascade_splits[0] = 123.0
    st = lib.uh_shadow_cascades((C.c_float * 16)(*view), (C.c_float * 16)(*proj), near, far, (C.c_float * 3)(*sun), C.byref(out))
    return st, out


def test_cascades_refuse_degenerate_inputs():
    c = cam.Camera((0.0, 2.0, 5.0), (0.0, 0.0, 0.0), 60.0, 1.5, 0.1, 100.0)
    V, P = cam.to_glam(c.get_view()).tolist(), cam.to_glam(c.get_projection()).tolist()
    ok, _ = _call(V, P, 0.1, 100.0, (0.3, -1.0, 0.2))
    assert ok == 0
    nan, inf = float("nan"), float("inf")
    bad = [(V, P, 0.0, 100.0, (0.3, -1, 0.2)), (V, P, -1.0, 100.0, (0.3, -1, 0.2)), (V, P, 1.0, 1.0, (0.3, -1, 0.2)),
           (V, P, 2.0, 1.0, (0.3, -1, 0.2)), (V, P, nan, 100.0, (0.3, -1, 0.2)), (V, P, 0.1, inf, (0.3, -1, 0.2)),
           (V, P, 0.1, 100.0, (nan, -1, 0.2)), (V, P, 0.1, 100.0, (0, 0, 0)), (V, P, 0.1, 100.0, (0, 1, 0)), (V, P, 0.1, 100.0, (0, -3, 0)),
           ([0.0] * 16, P, 0.1, 100.0, (0.3, -1, 0.2)), (V[:5] + [inf] + V[6:], P, 0.1, 100.0, (0.3, -1, 0.2)),
           (V, [nan] + P[1:], 0.1, 100.0, (0.3, -1, 0.2))]
    for args in bad:
        st, out = _call(*args)
        assert st == 1, args
        assert out.cascade_splits[0] == 123.0, "a refusal leaves *out untouched"


def test_set_params_rejects_without_a_device_context():
    lib = rr.load_library()
    lib.uh_set_shadowmap_params.argtypes = [C.c_void_p, C.c_void_p]
    lib.uh_read_shadow_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.uh_get_shadow_map_stats.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.uh_set_shadowmap_params(None, None) == 1
    assert lib.uh_read_shadow_map(None, 0, None) == 1
    assert lib.uh_get_shadow_map_stats(None, None) == 1


# ---- the numpy rasteriser's known answers -----------------------------------------------------------------------------------------
def _meshes(tris, world=None):
    """one mesh per list of (3, 3) world-space triangles"""
    v = np.zeros(3 * len(tris), dtype=rr.types.VERTEX_DTYPE)
    v["pos"][:, :3] = np.asarray(tris, np.float32).reshape(-1, 3)
    return [dict(vertices=v, indices=np.arange(3 * len(tris), dtype=np.uint32), world=rr.identity3x4() if world is None else world)]


def _ortho_vp(half=1.0):
    """x, y in [-half, half] to NDC, z_ndc = 0.5 - z / 4 (orthographic_rh(-h, h, -h, h, -2, 2) after an identity view)"""
    m = np.zeros(16, np.float32)
    m[0] = m[5] = np.float32(1.0 / half)
    m[10], m[14], m[15] = np.float32(-0.25), np.float32(0.5), np.float32(1.0)
    return m


def _layer(tris, S, vp=None):
    return sr.rasterise(sr.records_for(_meshes(tris), _ortho_vp() if vp is None else vp, S), S)


def test_quad_facing_the_light_covers_exactly_the_centres_inside_it():
    S = 64
    x0, x1, y0, y1, z = -0.5, 0.25, -0.3, 0.6, 0.4
    quad = [[(x0, y0, z), (x1, y0, z), (x1, y1, z)], [(x0, y0, z), (x1, y1, z), (x0, y1, z)]]
    d = _layer(quad, S)
    cx = (np.arange(S) + 0.5) / S * 2 - 1           # NDC x of texel centres
    cy = 1 - (np.arange(S) + 0.5) / S * 2            # row 0 at NDC y = +1
    inside = ((cy[:, None] > y0) & (cy[:, None] < y1)) & ((cx[None, :] > x0) & (cx[None, :] < x1))
    assert np.array_equal(d < 1.0, inside)
    assert np.all(d[inside] == np.float32(0.5 - z / 4))  # constant analytic depth


def test_split_quad_has_no_hole_and_no_double_coverage():
    S = 97
    rng = np.random.default_rng(3)
    for _ in range(20):
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))  # a convex quad (b and d on either side of the diagonal a c), corners beyond the map
        p = np.stack([np.cos(ang), np.sin(ang)], -1) * rng.uniform(0.3, 1.3) + rng.uniform(-0.3, 0.3, 2)  # on one circle: convex
        z = rng.uniform(-1.5, 1.5, 4)
        a, b, c, d4 = [(p[i, 0], p[i, 1], z[i]) for i in range(4)]
        cnt = np.zeros((S, S), np.int64)
        for t in ([a, b, c], [a, c, d4]):
            for rec in sr.records_for(_meshes([t]), _ortho_vp(), S):
                x0, x1, y0, y1 = rec[3]
                py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
                X, Y, zz, _ = rec
                Px, Py = px * 256 + 128, py * 256 + 128
                e = [(X[(k + 2) % 3] - X[(k + 1) % 3]) * (Py - Y[(k + 1) % 3]) - (Y[(k + 2) % 3] - Y[(k + 1) % 3]) * (Px - X[(k + 1) % 3]) for k in range(3)]
                tl = [sr._top_left(X[(k + 2) % 3] - X[(k + 1) % 3], Y[(k + 2) % 3] - Y[(k + 1) % 3]) for k in range(3)]
                cov = np.ones(px.shape, bool)
                for k in range(3):
                    cov &= (e[k] > 0) | ((e[k] == 0) & tl[k])
                np.add.at(cnt, (py[cov], px[cov]), 1)
        assert cnt.max() <= 1, "a texel centre on the shared diagonal is covered twice"
        # the union is the quad: every centre strictly inside it (by a float64 test, away from its edges) is covered
        P = np.stack(np.meshgrid((np.arange(S) + 0.5) / S * 2 - 1, 1 - (np.arange(S) + 0.5) / S * 2), -1)
        inner = np.ones((S, S), bool)
        q = p[[0, 1, 2, 3, 0]]
        for k in range(4):
            e = q[k + 1] - q[k]
            side = e[0] * (P[..., 1] - q[k, 1]) - e[1] * (P[..., 0] - q[k, 0])
            orient = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
            inner &= side * np.sign(orient) > 1e-3
        assert np.all(cnt[inner] == 1), "a hole inside the quad"


def test_straddling_triangle_keeps_only_its_inside_depths():
    S = 64
    tri = [[(-0.9, -0.9, 3.0), (0.9, -0.9, 3.0), (0.0, 0.9, -3.0)]]  # z_ndc from -0.25 to 1.25 across the triangle
    d = _layer(tri, S)
    got = d[d < 1.0]
    assert got.size > 0 and got.min() >= 0.0 and got.max() <= 1.0
    # the covered rows are those whose interpolated depth lies in [0, 1]: the band in the middle, not the two ends
    rows = np.nonzero((d < 1.0).any(axis=1))[0]
    full = _layer([[(-0.9, -0.9, 0.0), (0.9, -0.9, 0.0), (0.0, 0.9, 0.0)]], S)
    frows = np.nonzero((full < 1.0).any(axis=1))[0]
    assert rows.min() > frows.min() and rows.max() < frows.max()


def test_guard_band_clip_keeps_a_huge_floor_watertight():
    """a floor 10^4 times the cascade: every vertex beyond the guard band, clipped in float, still covers every texel exactly"""
    S = 33
    big = 1.0e4
    quad = [[(-big, -big, 0.5), (big, -big, 0.5), (big, big, 0.5)], [(-big, -big, 0.5), (big, big, 0.5), (-big, big, 0.5)]]
    d = _layer(quad, S)
    assert np.all(d == np.float32(0.5 - 0.5 / 4))
    assert all(len(r[0]) == 3 for r in sr.records_for(_meshes(quad), _ortho_vp(), S))

"""Shared by test_gpu_motion.py and test_gpu_denoise_motion.py: the moving scene (an emissive floor, a small isosurface mesh, a wall and a
"panel" of 4 x 4 cells facing the camera at depth 4 - the isosurface mesh lies before the wall and the panel in the vertex table, so an
update that changes its count shifts their vertex_base) on the denoiser tests' Rig. Not a test module."""
import numpy as np

import motion_reference as mr
import rust_renderer_amd as rr
from rust_renderer_amd.scenes import Scene, quad
from test_gpu_denoise import Rig

F = np.float32
FLOOR, ISO, WALL, PANEL = range(4)
SIZES = [(67, 45), (40, 24)]
EXTENT = 40.0  # the floor's and the wall's width: the scene's extent
PANEL_WORLD = rr.transform3x4((1.0, 1.0, 1.0), (0.0, 1.4, 0.0))
ISO_WORLD = rr.transform3x4((0.04, 0.04, 0.04), (-3.3, 0.0, 0.0))
ISO_RES, ISO_LO, ISO_HI, ISO_TIME = 10, 8.0, 32.0, 1.0


def panel_mesh():
    """5 x 5 shared vertices, 32 triangles, 3 x 2 units around the object-space origin, facing +z"""
    v, idx = quad((-1.5, -1.0, 0.0), (3.0, 0.0, 0.0), (0.0, 2.0, 0.0), nu=4, nv=4)
    assert len(v) == 25 and len(idx) == 96
    return v, idx


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(np.float32)


def mapped(vertices, a3x4):
    """the vertices with their positions under the affine map, rounded to float32 as the device receives them"""
    out = vertices.copy()
    out["pos"][:, :3] = mr.affine(a3x4, vertices["pos"][:, :3]).astype(np.float32)
    return out


class MotionRig(Rig):
    """the moving scene on a renderer; shoot() path-traces a frame and renders the G-buffer (cast or rasterised) with the motion bit,
    both with view.rebuild_tlas = 1"""

    def __init__(self, size, raster=False):
        self.size, self.raster = size, raster
        cam = rr.camera.Camera((0.0, 1.5, 4.0), (0.0, 1.0, -3.0), 60.0, size[0] / size[1], 0.01, 1000.0)
        self.scene = Scene("motion", [], [], cam, dict(sky_enabled=1))
        g = self.gpu = rr.Renderer(*size)
        white = g.default_diffuse_map()
        lambert = lambda *rgb: rr.make_material(rr.LAMBERTIAN, 0.0, rgb + (1.0,), diffuse_map=white)
        fv, fi = quad((-20.0, 0.0, 10.0), (40.0, 0.0, 0.0), (0.0, 0.0, -13.0), nu=4, nv=4)
        assert g.add_mesh(fv, fi, rr.make_material(rr.DIFFUSE_LIGHT, 0.0, (1.0, 1.0, 1.0, 1.0), diffuse_map=white)) == FLOOR
        mesh, tris = g.add_isosurface_mesh(ISO_RES, ISO_LO, ISO_HI, ISO_TIME, material=lambert(0.8, 0.6, 0.3), world3x4=ISO_WORLD)
        assert mesh == ISO and tris > 0
        wv, wi = quad((-20.0, 0.0, -3.0), (40.0, 0.0, 0.0), (0.0, 2.6, 0.0), nu=4, nv=4)  # low: the upper rows see the sky
        assert g.add_mesh(wv, wi, lambert(0.3, 0.3, 0.3)) == WALL
        self.panel_v, self.panel_i = panel_mesh()
        assert g.add_mesh(self.panel_v, self.panel_i, lambert(0.7, 0.8, 0.9), PANEL_WORLD) == PANEL
        g.initialize_raytracing()
        self.shots = 0
        self.prev_pv = None

    def mask(self, motion=True):
        return rr.HYBRID_GBUFFER | (rr.HYBRID_MOTION if motion else 0) | (rr.HYBRID_GBUFFER_RASTER if self.raster else 0)

    def view(self, shift=0.0):
        v = super().view(shift)
        v.rebuild_tlas = 1
        return v

    def gbuffer(self, v=None, motion=True):
        """a G-buffer pass alone; returns (position, mesh index image, geometry mask, motion image or None)"""
        v = self.view() if v is None else v
        self.gpu.render_hybrid(v, self.mask(motion))
        pos = self.gpu.read_hybrid(rr.HYBRID_POSITION)
        return pos, self.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3], pos[..., 3] != 0, (self.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE) if motion else None)

    def shoot(self, v, spp=1, gbuffer=True, motion=True):
        v.samples_per_frame = v.total_samples = spp
        v.time = 0.25 + 0.125 * self.shots
        self.shots += 1
        self.gpu.render_frame(v, rr.PASS_REFERENCE_PT)
        if gbuffer:
            self.gpu.render_hybrid(v, self.mask(motion))
        return v

    def inputs(self):
        return super().inputs() + (self.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE),)

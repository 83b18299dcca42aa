"""GPU: the three passes that came after test_gpu_hybrid_sizes.py - the motion image, uh_denoise and UH_HYBRID_TAA, whose kernels run one
lane per pixel in blocks of 4 rows of 64 - at frame sizes where such kernels go wrong: one pixel, one column, one row, frames narrower
than TAA's 3 x 3 box, the 7 x 7 variance window and the a-trous step of 16, exactly one block, one pixel into a second block column and
row, and five block columns. Three calls per size on the moving scene of motion_util.py, with the cast and the rasterised G-buffer: the
camera at rest; the camera 0.3 to the side and the panel moved rigidly; the isosurface at another topology. Every call is held to
motion_reference.py, denoise_motion_reference.py and taa_reference.py, and a second renderer without UH_DENOISE_MOTION, on which only
the camera moves, to denoise_reference.py, with the tolerances of the tests that hold them at the usual sizes.

Wherever a frame has 64 pixels or more, the camera's step leaves both filters pixels that keep their history and pixels that lose it:
the denoiser the wall that the panel uncovers and the strip that enters the frame, UH_HYBRID_TAA, which has no rejection test, that
strip."""
import numpy as np
import pytest

import denoise_motion_reference as dmr
import denoise_reference as dr
import motion_reference as mr
import rust_renderer_amd as rr
import taa_reference as tr
from motion_util import EXTENT, ISO, PANEL, PANEL_WORLD, rot
from temporal_gpu_util import TemporalRig, hold_denoise, hold_expf, hold_taa
from test_gpu_denoise import params
from test_gpu_motion import MOTION_HELD, assert_verbatim, compose

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (1, 45), (67, 1), (64, 4), (65, 5), (257, 3), (130, 70)]
FORMS = [pytest.param(False, id="cast"), pytest.param(True, id="raster")]
SHIFT = 0.3
# the panel's second place: half a unit to the other side than the camera's step, turned a little in its own plane - the wall it
# uncovers is several pixels wide at every size
MOVED = rr.transform3x4((1.0, 1.0, 1.0), (-0.5, 1.4, 0.0), rot(0.0, 0.0, 0.03))


def camera(w, h):
    """(eye, target), vertical field of view: a camera of this aspect on motion_util's scene. A frame of a few rows with 60 degrees of
    height would be some 170 degrees wide, and a sideways step would move nothing in it by a texel; such a frame gets the height that
    makes it 60 degrees WIDE, a strip of MotionRig's view. With three rows or more the strip looks at the wall's upper edge (2.6 high,
    7 away), so that its upper rows see the sky and its lower ones the wall, with the panel's upper part (2.4 high, 4 away) before it
    in the middle columns; a single row looks where MotionRig's camera looks. The others keep MotionRig's camera, whose upper rows
    see the sky"""
    eye = (0.0, 1.5, 4.0)
    if w >= 8 * h:
        fov = float(np.degrees(2.0 * np.arctan(np.tan(np.radians(30.0)) * h / w)))
        return (eye, (0.0, 2.6 if h >= 3 else 1.0, -3.0)), fov
    return (eye, (0.0, 1.0, -3.0)), 60.0


def verbatim(pos, motion, where, w):
    """test_gpu_motion.assert_verbatim, which also asks that `where` is not empty: one pixel may well be all panel"""
    if where.any():
        assert_verbatim(pos, motion, where, w)


@pytest.mark.parametrize("raster", FORMS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_temporal_passes_at_an_awkward_size(w, h, raster):
    r = TemporalRig((w, h), raster, *camera(w, h))
    plain = TemporalRig((w, h), raster, *camera(w, h))  # no UH_DENOISE_MOTION, and only its camera moves
    dn = params(flags=rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE | rr.DENOISE_MOTION)
    dn_plain = params(flags=rr.DENOISE_TEMPORAL | rr.DENOISE_DEMODULATE)
    taa = r.gpu.set_taa_params(flags=rr.TAA_CLAMP | rr.TAA_MOTION)
    ref_dn, ref_plain, ref_taa = dmr.MotionDenoiser(), dr.Denoiser(), tr.Taa()
    worst = worst_colour = 0.0
    for call in range(3):
        if call == 1:
            r.gpu.set_instance_transform(PANEL, MOVED)
        elif call == 2:
            r.gpu.update_isosurface_mesh(ISO, 3.0)
            r.gpu.build_acceleration()
        v = r.step(SHIFT if call else 0.0, dn)
        # the motion image
        pos, motion, mesh = r.gpu.read_hybrid(rr.HYBRID_POSITION), r.gpu.read_hybrid(rr.HYBRID_MOTION_IMAGE), r.gpu.read_hybrid(rr.HYBRID_PBR)[..., 3]
        geo = pos[..., 3] != 0
        assert geo.any()
        if h >= 3:
            assert not geo.all(), "sky and geometry"
        assert not motion[~geo].any(), "not geometry: (0, 0, 0, 0)"
        panel, iso = geo & (mesh == PANEL), geo & (mesh == ISO)
        assert panel.any(), "the panel is on screen at every size"
        ms = r.gpu.motion_stats()
        assert (ms.meshes_rigid, ms.meshes_deformed, ms.meshes_none) == (call == 1, 0, call == 2)
        assert (ms.pixels_with, ms.pixels_without) == (geo.sum() - (iso.sum() if call == 2 else 0), iso.sum() if call == 2 else 0)
        if call == 1:
            want = mr.affine(compose(PANEL_WORLD, mr.inverse3x4(MOVED)), pos[..., :3])
            assert float(np.abs(want[panel] - pos[..., :3][panel]).max()) > 0.05, "the panel moved"
            assert (motion[..., 3][panel] == 1).all()
            e = float(np.abs(motion[..., :3][panel].astype(np.float64) - want[panel]).max()) / EXTENT
            print(f"motion: largest |device - float64| / extent over {panel.sum()} pixels: {e:.3e} (held {MOTION_HELD:.3e})")
            assert e <= MOTION_HELD
            verbatim(pos, motion, geo & ~panel, 1.0)
        elif call == 2:
            verbatim(pos, motion, iso, 0.0)
            verbatim(pos, motion, geo & ~iso, 1.0)
        else:
            verbatim(pos, motion, geo, 1.0)
        if (w, h) == (130, 70):
            assert iso.sum() >= 4, "the isosurface is on screen"
        # the denoiser that follows the motion image
        want, im, a, b = hold_denoise(r, ref_dn, r.inputs(), v, dn, dmr.params_of, call)
        worst, worst_colour = max(worst, a), max(worst_colour, b)
        kept = want["kept"]
        if call == 0:
            assert not kept.any()
        elif call == 1 and w * h >= 64:
            print(f"call {call}: history kept on {kept.sum()} of {geo.sum()} geometry pixels")
            assert kept.any() and not kept[geo].all(), "kept and dropped histories both occur"
        if call == 2:
            assert not kept[iso].any(), "no correspondence: no history"
        # the resolve
        wt, _, _, n = hold_taa(r, ref_taa, v, taa)
        if call == 0:
            assert (n == 1).all() and wt["history_pixels"] == 0
        elif w * h >= 64:
            assert wt["history_pixels"] > 0 and (n > 1.5).any()
            if call == 1:
                assert wt["history_pixels"] < w * h, "a strip of the frame has no history"
        if call == 2:
            assert (n[iso] == 1).all()
        # the denoiser without the flag, on the camera-only calls
        if call < 2:
            v2 = plain.step(SHIFT if call else 0.0, dn_plain, taa=False)
            want, im, a, b = hold_denoise(plain, ref_plain, plain.inputs()[:5], v2, dn_plain, dr.params_of, call)
            worst, worst_colour = max(worst, a), max(worst_colour, b)
            kept, geo2 = want["kept"], want["geometry"]
            if call == 0:
                assert not kept.any()
            elif w * h >= 64:
                print(f"call {call}, no motion flag: history kept on {kept.sum()} of {geo2.sum()} geometry pixels")
                assert kept.any() and not kept[geo2].all(), "kept and dropped histories both occur"
    hold_expf(worst, worst_colour)

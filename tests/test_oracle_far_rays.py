"""CPU: the oracle's tree walk against its own brute force for rays that start far from small geometry lying in a coordinate
plane. The oracle's boxes are padded by 1e-4 + 1e-5 |coord|, an absolute amount near a coordinate plane, while the rounding of
the slab test and of the triangle test grows with the distance to the ray's origin: from a few thousand units on, a slab test
that does not allow for it culls triangles the triangle test accepts, and the reference most GPU tests compare against loses
hits (DESIGN.md "Arithmetic contract"). No GPU needed."""
import numpy as np
import pytest

import oracle_api as oa
from util import FAR_DISTANCES, FAR_SCENES, far_rays, far_scene

N_RAYS = 40_000
MISS = 0xFFFFFFFF


def _compare(kind, distance, normalised, seed):
    scene = far_scene(kind)
    tree = scene.upload(oa.OracleRenderer(8, 8))
    brute = scene.upload(oa.OracleRenderer(8, 8, brute_force=True))
    rays = far_rays(kind, distance, N_RAYS, seed, normalised)
    (tt, mt, pt), (tb, mb, pb) = tree.trace_closest(rays), brute.trace_closest(rays)
    front = int((mb == 0).sum())
    differ = int(((tt.view(np.uint32) != tb.view(np.uint32)).any(axis=1) | (mt != mb) | (pt != pb)).sum())
    print(f"{kind} D={distance:g} normalised={normalised}: brute force hits mesh 0 with {front} of {N_RAYS} rays, the tree differs on {differ}, "
          f"misses {int(((mt == MISS) & (mb != MISS)).sum())} outright")
    assert front >= 0.3 * N_RAYS, "the rays must hit the surface they are aimed at, or the comparison is vacuous"
    assert np.array_equal(mt, mb) and np.array_equal(pt, pb)
    assert np.array_equal(tt.view(np.uint32), tb.view(np.uint32)), "t / u / v of the tree walk must equal brute force bit for bit"
    assert np.array_equal(tree.trace_any(rays).astype(bool), mb != MISS)


@pytest.mark.parametrize("distance", FAR_DISTANCES)
@pytest.mark.parametrize("kind", FAR_SCENES)
def test_oracle_tree_equals_brute_force_far_away(kind, distance):
    _compare(kind, distance, False, seed=1000 + FAR_SCENES.index(kind) * 16 + FAR_DISTANCES.index(distance))


@pytest.mark.parametrize("distance", [d for d in FAR_DISTANCES if d <= 3e3])
@pytest.mark.parametrize("kind", FAR_SCENES)
def test_oracle_tree_equals_brute_force_far_away_unit_directions(kind, distance):
    _compare(kind, distance, True, seed=2000 + FAR_SCENES.index(kind) * 16 + FAR_DISTANCES.index(distance))

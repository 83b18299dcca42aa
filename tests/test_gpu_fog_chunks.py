"""GPU: the fog pass's persistent walk (k_fog_trace<0|1|2>) at a frame where a wave comes back for several chunks of 64 items, as
tests/test_gpu_walk_chunks.py holds the other walks: option "trace_blocks_per_cu" = 1, the slab scene at 131 x 97 and 32 steps - 406,624
items, 6.2 grids of at most 65,536 lanes for the layouts that walk one sample per item. The masks and totals are bit for bit the
restatement's (tests/fog_reference.py), and the masks of 1 block per CU are those of the default grid, device against device. Layout 2
walks one pixel per item, 12,707 items, one chunk per wave at this size; a frame that refills it is beyond the restatement, and it is
held to the other two layouts' masks here."""
import numpy as np
import pytest

import fog_reference as fog
from test_gpu_fog import MASK, World

pytestmark = pytest.mark.gpu

WIDE, TALL, STEPS = 131, 97, 32
LANES = 65536  # 256 CUs x 1 block x 256 lanes at most


@pytest.fixture(scope="module")
def worlds():
    one, default = (World(fog.slab_scene(WIDE, TALL), WIDE, TALL, fog.slab_view, max_distance=fog.SLAB_MAX_DISTANCE, density=0.08) for _ in range(2))
    one.gpu.set_option("trace_blocks_per_cu", 1)
    default._masks = one._masks  # the same scene, view and G-buffer (compared before reuse): one restatement serves both
    return one, default


@pytest.mark.parametrize("order", [0, 1, 2])
def test_every_wave_refills_and_the_masks_equal_the_restatement(worlds, order):
    assert WIDE * TALL * STEPS == 406624 and WIDE * TALL * STEPS >= 6 * LANES
    got = []
    for w in worlds:
        v = w.view()
        w.gpu.set_option("fog_order", order)
        try:
            w.render(v, steps=STEPS, blur_radius=2)
            _, mask, _, _ = w.check(v)
        finally:
            w.gpu.set_option("fog_order", 2)
        s = w.gpu.fog_stats()
        assert s.pixels == WIDE * TALL and s.rays == WIDE * TALL * STEPS and 0 < s.lit < s.rays
        got.append(mask)
    assert np.array_equal(got[0], got[1]), "1 block per CU against the default grid"
    assert (got[0] == 0).any() and ((got[0] != 0) & (got[0] != np.uint32(0xFFFFFFFF))).any() and (got[0] >> 31).any()
    assert np.array_equal(worlds[0].gpu.read_hybrid(MASK), got[0])

"""GPU: the glass pass's rounds at a frame where the persistent walk refills. With option "trace_blocks_per_cu" = 1 a persistent grid
holds at most 65,536 lanes; the nested boxes at 263 x 167 put 87,842 rays into round 0 and, every chain going on, 87,842 into round 1: the
walk takes more than one chunk per wave from the first queue and from the second, which the bend kernel of round 0 filled. As
tests/test_gpu_glossy_chunks.py does for the glossy pass, against the restatement (tests/glass_reference.py)."""
import numpy as np
import pytest

import glass_reference as gs
import rust_renderer_amd as rr
from test_gpu_glass import World

pytestmark = pytest.mark.gpu


def test_both_queues_refill_in_the_nested_boxes():
    Ww, Hh = gs.WALK_NESTED_SIZE
    w = World(gs.nested_boxes_scene(), Ww, Hh)
    w.gpu.set_option("trace_blocks_per_cu", 1)
    v = w.view()
    w.render(v, rr.HYBRID_FRAME)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v, max_events=8)
    got = w.check(v, plain)
    s = w.gpu.glass_stats()
    print(gs.integers(s), got["ch"]["rounds"])
    n = Ww * Hh
    assert got["ch"]["rounds"][:4] == [2 * n, 2 * n, n, 0] and 2 * n == 87842 and gs.WALK_LANES < 2 * n <= 8 * gs.WALK_LANES, "rounds 0 and 1 take more than one chunk"
    assert got["exact"].all(), "no chain misses: every pixel is held bit for bit"
    assert (got["counts"] == (0, 0, 2, 0)).all() and (got["events"] == (3, 2, 0, 0)).all()
    assert s.chains == 2 * n and s.segments == 5 * n and s.events == 3 * n and s.misses == 0 and s.cut == 0
    assert (np.abs(got["radiance"][..., :3].astype(np.float64) - 1.0) <= np.spacing(np.float32(1.0))).all()

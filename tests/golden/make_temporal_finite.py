"""Writes temporal_finite.npz: the images of tests/temporal_cases.py's finite sequences through the three temporal restatements
(denoise_reference, denoise_motion_reference, taa_reference). It was run once at the commit BEFORE the restatements got their rule for
non-finite input; test_denoise_cpu.py and test_taa_cpu.py hold today's restatements to these bits. Running it again at a later commit
only records that commit against itself.

  python tests/golden/make_temporal_finite.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
sys.path[:0] = [p for p in os.environ.get("TEMPORAL_RESTATEMENTS", "").split(os.pathsep) if p]  # another directory's restatements first

import denoise_motion_reference as dmr  # noqa: E402
import denoise_reference as dr  # noqa: E402
import taa_reference as tr  # noqa: E402
import temporal_cases as tc  # noqa: E402

if __name__ == "__main__":
    cases = dict(tc.finite_denoise_cases(dr, dmr), **tc.finite_taa_cases(tr))
    np.savez_compressed(os.path.join(HERE, "temporal_finite.npz"), **cases)
    print(len(cases), "arrays from", dr.__file__)
